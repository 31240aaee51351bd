"""The definition of nmod_pair_rows_count / nmod_pair_rows_fill / nmod_pair_linkage (K18, include/nanomod_hip.h) restated for the tests:
the rows by a plain loop over the reads, the two-stage statistic in float64 in the header's order of operations (the reductions by
math.fsum), its gates, the full four-weight model by EM, and the seeded pairs that the CPU pin (tests/test_site_linkage.py) and the
GPU tests (tests/test_site_linkage_gpu.py) share.  Written from the header's text; the reference project has no such step.

Stage 1 is stoich_ref's: the margins are stoich_ref.row's pi of the two rows (a read with either score invalid is masked out of both).
Stage 2 per read: u_a, u_b = K14's u at the margins with the sign of the side, v = u_a u_b; an evaluation at D is
    dv = max(D v, -1),  w = v / (1 + dv),  S = sum w,  Q = sum w^2,  g = sum log1p(dv).

The gates of stage 2 are built from stoich_ref's constants and nothing else (the same arithmetic: a division and a few rounded
operations per read, one log1p, t from two expm1 libraries), AT GIVEN MARGINS: row(..., margins=(pa, pb)) restates stage 2 at the
margins it is handed, so that a comparison does not have to allow for the margins' own deviation, which K14's gates already bound.
    v: a relative error C_T EPS of t moves u by C_T EPS u^2 / t, i.e. u relatively by C_T EPS u / t, and v relatively by
       rv = C_T EPS (|u_a| / t_a + |u_b| / t_b);  w = v / (1 + D v) moves by rv |w| / (1 + dv), log1p(D v) by rv |D w|.
    S: C_SUM n EPS sum|w| (the sum and the handful of rounded operations per term) + sum rv |w| / (1 + dv).
    g: EPS (C_SUM n + C_LOG) sum|log1p(dv)| + sum rv |D w|.
    D^ (interior): tol + 2 EPS + err(S) / Q;  g(D^): err(g) + Q gate(D^)^2 / 2 (g' = S is 0 at the root);
    an end of the interval: tol + 2 EPS + (err(g at the end) + err(g(D^))) / |S at the end|;
    stat = 2 g(D^): twice its error;  p_indep: between the tails at stat -+ that, widened by C_ERFC EPS;
    r = D^ / sqrt((pa qa)(pb qb)): gate(D^) over the root + C_ROUND EPS |r|."""
import functools
import math

import numpy as np

import stoich_ref as F

TOO_FEW, FLAT, NOT_CONVERGED, AT_MIN, AT_MAX, TOO_LARGE, DEGENERATE = 1, 2, 4, 8, 16, 32, 64
FIELDS = ('pa', 'pb', 'd', 'd_lo', 'd_hi', 'r', 'stat', 'p_indep')
STAGE2 = ('d', 'd_lo', 'd_hi', 'r', 'stat', 'p_indep')
SMALL, WAVE = F.SMALL, F.WAVE
STAGE = 6144                                          # doubles of a row the workgroup form stages (site_linkage.hip: kLkStage)
POS_MASK = (1 << 40) - 1
DBL_MAX, DBL_MIN, EPS = F.DBL_MAX, F.DBL_MIN, F.EPS
DEFAULTS = dict(min_reads=20, max_iter=60, tol=1e-12, ci_drop=F.ci_drop_of(0.95))


# ---- the rows
def pair_rows_ref(cs, start, roff, score, key, poff):
    """prow_off (int64[npairs + 1]), sa, sb (float64), read (int32): per pair the reads valid at both sites, in read order"""
    key = np.asarray(key, dtype=np.int64)
    npairs = int(poff[-1])
    rows = [[] for _ in range(npairs)]
    for r in range(len(cs)):
        b, n = int(roff[r]), int(roff[r + 1] - roff[r])
        if n <= 0:
            continue
        lo = np.searchsorted(key, (int(cs[r]) << 40) | int(start[r]), 'left')
        hi = np.searchsorted(key, (int(cs[r]) << 40) | (int(start[r]) + n - 1), 'right')
        valid = []
        for s in range(lo, hi):
            pos = int(key[s]) & POS_MASK
            i = int(start[r]) + n - 1 - pos if cs[r] & 1 else pos - int(start[r])
            if abs(score[b + i]) <= DBL_MAX:
                valid.append((s, float(score[b + i])))
        for x, (a, la) in enumerate(valid):
            reach = a + 1 + int(poff[a + 1] - poff[a])
            for bb, lb in valid[x + 1:]:
                if bb >= reach:
                    break
                rows[int(poff[a]) + (bb - a - 1)].append((r, la, lb))
    prow_off = np.zeros(npairs + 1, np.int64)
    prow_off[1:] = np.cumsum([len(x) for x in rows])
    flat = [t for x in rows for t in x]
    return dict(prow_off=prow_off, sa=np.array([t[1] for t in flat], np.float64), sb=np.array([t[2] for t in flat], np.float64),
                read=np.array([t[0] for t in flat], np.int32))


# ---- the statistic
def signed_u(w, p):
    t, plus = np.abs(w), w >= 0.0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        u = t / (1.0 - np.where(plus, 1.0 - p, p) * t)
    return np.where(plus, u, -u)


def evaluate(v, D, rv=None):
    """(S, Q, g) at D over the products v; with rv (the relative error of each v) also the error terms of the gates"""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        dv = np.maximum(D * v, -1.0)
        w = v / (1.0 + dv)
        lg = np.log1p(dv)
        e = dict(S=math.fsum(w), D=math.fsum(w * w), g=math.fsum(lg))
        if rv is not None and np.all(np.isfinite(w)) and np.all(np.isfinite(lg)):
            n = len(v)
            e['S_err'] = EPS * F.C_SUM * n * math.fsum(np.abs(w)) + math.fsum(rv * np.abs(w) / (1.0 + dv))
            e['g_err'] = EPS * (F.C_SUM * n + F.C_LOG) * math.fsum(np.abs(lg)) + math.fsum(rv * np.abs(D * w))
    return e


def solve(v, mode, a, b, ghat, drop, max_iter, tol):
    """stoich_ref.solve over the products: the bracketed iteration of the header with this evaluation"""
    x = a + 0.5 * (b - a)
    for k in range(1, max_iter + 1):
        e = evaluate(v, x)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            if mode == 0:
                right = e['S'] > 0.0
                xn = x + np.float64(e['S']) / np.float64(e['D'])
            else:
                h = 2.0 * (ghat - e['g'])
                right = h > drop if mode == 1 else h <= drop
                xn = x + np.float64(h - drop) / np.float64(2.0 * e['S'])
        a, b = (x, b) if right else (a, x)
        if xn != x and not (xn > a and xn < b):
            xn = a + 0.5 * (b - a)
        step = abs(xn - x)
        x = float(xn)
        if tol > 0.0 and (b - a <= tol or step <= tol):
            return x, k, False
    return x, max_iter, True


def _nan_row(n, status):
    r = {f: np.nan for f in FIELDS}
    r.update(n_valid=n, iters=0, status=status, gates=None)
    return r


def row(sa, sb, min_reads=20, max_iter=60, tol=1e-12, ci_drop=F.CI_DROP_95, margins=None, interval=True):
    """one pair by the header's definition: its outputs and `gates` (None without an estimate or for a DEGENERATE pair, whose outputs
    are constants).  margins: (pa, pb) to restate stage 2 at, instead of stage 1's"""
    sa, sb = np.asarray(sa, np.float64), np.asarray(sb, np.float64)
    if len(sa) > 16777215:
        return _nan_row(0, TOO_LARGE)
    both = (np.abs(sa) <= DBL_MAX) & (np.abs(sb) <= DBL_MAX)
    n = int(both.sum())
    if n < min_reads:
        return _nan_row(n, TOO_FEW)
    nan = np.full(len(sa), np.nan)
    ma, mb = np.where(both, sa, nan), np.where(both, sb, nan)      # a read that is not valid at both sites takes no part in either row
    wa, wb = F.signed_t(ma), F.signed_t(mb)
    if not math.fsum(np.abs(wa)) > 0.0 or not math.fsum(np.abs(wb)) > 0.0:
        return _nan_row(n, FLAT)
    ra = F.row(ma, min_valid=1, max_iter=max_iter, tol=tol, ci_drop=ci_drop, estimate_only=True)
    rb = F.row(mb, min_valid=1, max_iter=max_iter, tol=tol, ci_drop=ci_drop, estimate_only=True)
    nc = _margin_nc(wa, max_iter, tol) or _margin_nc(wb, max_iter, tol)
    pa, pb = (ra['pi'], rb['pi']) if margins is None else (float(margins[0]), float(margins[1]))
    out = dict(pa=pa, pb=pb, n_valid=n)
    if pa in (0.0, 1.0) or pb in (0.0, 1.0):
        out.update(d=0.0, d_lo=0.0, d_hi=0.0, r=np.nan, stat=0.0, p_indep=1.0, iters=0, status=DEGENERATE | (NOT_CONVERGED if nc else 0), gates=None)
        return out
    qa, qb = 1.0 - pa, 1.0 - pb
    ua, ub = signed_u(wa, pa), signed_u(wb, pb)
    v = ua * ub
    with np.errstate(divide='ignore', invalid='ignore'):
        rv = F.C_T * EPS * (np.where(wa != 0.0, np.abs(ua) / np.where(wa != 0.0, np.abs(wa), 1.0), 0.0) +
                            np.where(wb != 0.0, np.abs(ub) / np.where(wb != 0.0, np.abs(wb), 1.0), 0.0))
    d_min, d_max = -min(pa * pb, qa * qb), min(pa * qb, qa * pb)
    e_min, e_max = evaluate(v, d_min, rv), evaluate(v, d_max, rv)
    at_min = e_min['S'] <= 0.0
    at_max = not at_min and e_max['S'] >= 0.0
    iters = 0
    if at_min or at_max:
        d = d_min if at_min else d_max
    else:
        d, iters, c = solve(v, 0, d_min, d_max, 0.0, 0.0, max_iter, tol)
        nc = nc or c
    eh = evaluate(v, d, rv)
    gh = eh['g']
    stat = max(2.0 * gh, 0.0)
    lo_end, hi_end = 2.0 * (gh - e_min['g']) <= ci_drop, 2.0 * (gh - e_max['g']) <= ci_drop
    lo, hi = d_min, d_max
    if interval and not lo_end:
        lo, _, c = solve(v, 1, d_min, d, gh, ci_drop, max_iter, tol)
        nc = nc or c
    if interval and not hi_end:
        hi, _, c = solve(v, 2, d, d_max, gh, ci_drop, max_iter, tol)
        nc = nc or c
    root = math.sqrt((pa * qa) * (pb * qb))
    r = d / root
    p = max(math.erfc(math.sqrt(stat / 2.0)), DBL_MIN)

    interior = not (at_min or at_max)
    g_d = tol + 2.0 * EPS + eh['S_err'] / eh['D'] if interior else 0.0
    gh_err = eh['g_err'] + 0.5 * eh['D'] * g_d * g_d

    def g_end(x, fixed):
        if fixed:
            return 0.0
        ev = evaluate(v, x, rv)
        return tol + 2.0 * EPS + (ev['g_err'] + gh_err) / abs(ev['S'])
    tail = lambda s: max(math.erfc(math.sqrt(max(s, 0.0) / 2.0)), DBL_MIN)
    p_rng = (tail(stat + 2.0 * gh_err) * (1.0 - F.C_ERFC * EPS), tail(stat - 2.0 * gh_err) * (1.0 + F.C_ERFC * EPS))
    gates = dict(d=g_d, d_lo=g_end(lo, lo_end) if interval else 0.0, d_hi=g_end(hi, hi_end) if interval else 0.0, stat=2.0 * gh_err,
                 p_indep=p_rng, r=g_d / root + F.C_ROUND * EPS * abs(r))
    out.update(d=d, d_lo=lo, d_hi=hi, r=r, stat=stat, p_indep=p, iters=iters,
               status=(NOT_CONVERGED if nc else 0) | (AT_MIN if at_min else 0) | (AT_MAX if at_max else 0), gates=gates)
    return out


def _margin_nc(w, max_iter, tol):
    """whether K14's root of this row ends without its stop test holding (stoich_ref.row folds that into its status)"""
    if F.evaluate(w, 0.0)['S'] <= 0.0 or F.evaluate(w, 1.0)['S'] >= 0.0:
        return False
    return F.solve(w, 0, 0.0, 1.0, 0.0, 0.0, max_iter, tol)[2]


def pair_linkage(sa, sb, prow_off, margins=None, **opts):
    """every pair of the rows: a list of row() results; margins: (pa[npairs], pb[npairs]) to restate stage 2 at"""
    o = dict(DEFAULTS, **opts)
    out = []
    for j in range(len(prow_off) - 1):
        sl = slice(int(prow_off[j]), int(prow_off[j + 1]))
        m = None if margins is None or np.isnan(margins[0][j]) else (margins[0][j], margins[1][j])
        out.append(row(sa[sl], sb[sl], margins=m, **o))
    return out


def cells(pa, pb, d):
    """pi11, pi10, pi01, pi00 from the margins and the linkage"""
    qa, qb = 1.0 - pa, 1.0 - pb
    return pa * pb + d, pa * qb - d, qa * pb - d, qa * qb + d


# ---- the full model: four weights by EM
def full_stat(sa, sb, iters=5000, tol=1e-11):
    """twice the log-likelihood ratio of the full four-weight model against independence, both maximised: EM from the independence
    table at the marginal estimates.  Returns (stat, converged)"""
    sa, sb = np.asarray(sa, np.float64), np.asarray(sb, np.float64)
    la = np.stack([np.where(sa >= 0.0, np.exp(-np.abs(sa)), 1.0), np.where(sa >= 0.0, 1.0, np.exp(-np.abs(sa)))])     # state 0, state 1
    lb = np.stack([np.where(sb >= 0.0, np.exp(-np.abs(sb)), 1.0), np.where(sb >= 0.0, 1.0, np.exp(-np.abs(sb)))])
    joint = np.stack([la[x] * lb[y] for x in (0, 1) for y in (0, 1)])                                                    # 00, 01, 10, 11
    pa = F.row(sa, min_valid=1, estimate_only=True)['pi']
    pb = F.row(sb, min_valid=1, estimate_only=True)['pi']
    indep = np.array([(1 - pa) * (1 - pb), (1 - pa) * pb, pa * (1 - pb), pa * pb])
    l0 = float(np.sum(np.log(indep @ joint)))
    w = np.clip(indep, 1e-6, None)
    w /= w.sum()
    converged = False
    for _ in range(iters):
        post = w[:, None] * joint
        post /= post.sum(axis=0)
        new = post.mean(axis=1)
        converged = float(np.abs(new - w).max()) < tol
        w = new
        if converged:
            break
    return 2.0 * (float(np.sum(np.log(w @ joint))) - l0), converged


# ---- seeded pairs
def simulate_pair(rng, n, sep, pa, pb, d=0.0):
    """the window sums of n reads over two sites whose hidden states follow the joint law (pa, pb, d): unit-spread levels `sep` apart"""
    p11, p10, p01, p00 = cells(pa, pb, d)
    state = rng.choice(4, size=n, p=[p00, p01, p10, p11])
    za, zb = state >= 2, (state & 1) == 1
    xa, xb = rng.normal(size=n) + sep * za, rng.normal(size=n) + sep * zb
    return sep * xa - 0.5 * sep * sep, sep * xb - 0.5 * sep * sep


def _csr(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r[0]) for r in rows])
    cat = lambda k: np.concatenate([r[k] for r in rows]) if rows else np.zeros(0)
    return cat(0), cat(1), off


MIN_READS = 20
# a row of one read, min_reads - 1 and min_reads, the sub-wave / wave step, the wave / workgroup step, and the staged limits of the
# workgroup form (both t rows staged up to STAGE / 2 reads, the products up to STAGE)
PARITY_LENGTHS = (1, MIN_READS - 1, MIN_READS, SMALL - 1, SMALL, SMALL + 1, WAVE, WAVE + 1, STAGE // 2, STAGE // 2 + 1, STAGE, STAGE + 1)


@functools.lru_cache(maxsize=None)
def parity_batch():
    """(sa, sb, prow_off): two pairs of every length of PARITY_LENGTHS, separations, shares and linkage rotating"""
    rng = np.random.default_rng(1801)
    rows = []
    for i, n in enumerate(PARITY_LENGTHS):
        for j in range(2):
            sep = (3.0, 1.5, 2.0)[(i + j) % 3]
            pa, pb = ((0.3, 0.5), (0.5, 0.5), (0.2, 0.3))[(i + 2 * j) % 3]
            rows.append(simulate_pair(rng, n, sep, pa, pb, (0.0, 0.08, -0.05)[(i + j) % 3]))
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def planted_batch():
    """(sa, sb, prow_off, names): a pair for every status bit but TOO_LARGE, rows with NaN and +-inf scores on either side, signed
    zeros, and perfectly linked / perfectly exclusive calls (the ends of the range)"""
    rng = np.random.default_rng(1802)
    nan, inf = np.nan, np.inf
    rows, names = [], []

    def add(name, a, b):
        rows.append((np.asarray(a, np.float64), np.asarray(b, np.float64)))
        names.append(name)
    a, b = simulate_pair(rng, 60, 3.0, 0.4, 0.4, 0.1)
    add('plain', a, b)
    add('too_few', a[:5], b[:5])
    a2, b2 = a.copy(), b.copy()
    a2[::3] = nan
    b2[1::3] = inf
    b2[2] = -inf
    add('invalid_mix', a2, b2)
    a3 = a[:30].copy()
    a3[:12] = nan
    add('too_few_by_invalid', a3, b[:30])
    add('flat_a', np.zeros(40), b[:40])
    add('flat_b', a[:40], np.where(np.arange(40) % 2 == 0, 0.0, -0.0))
    add('degenerate_a0', -np.abs(a[:40]) - 1.0, b[:40])
    add('degenerate_b1', a[:40], np.abs(b[:40]) + 1.0)
    s = np.where(rng.random(80) < 0.5, 40.0, -40.0)
    add('at_max', s, s)                                   # perfect calls, perfectly linked: D at the upper end
    add('at_min', s, -s)                                  # perfectly exclusive: D at the lower end
    t = np.where(rng.random(80) < 0.3, 40.0, -40.0)
    add('perfect_calls', s, np.where(rng.random(80) < 0.7, s, t))
    add('big_scores', np.where(a[:40] > 0, 1e300, -800.0), b[:40])
    a4, b4 = simulate_pair(rng, 300, 2.0, 0.3, 0.3, 0.1)
    a4[5] = nan
    b4[7] = -inf
    add('wave_invalid', a4, b4)
    a5, b5 = simulate_pair(rng, 1500, 1.5, 0.3, 0.5, -0.04)
    a5[100] = inf
    add('block_invalid', a5, b5)
    sa, sb, off = _csr(rows)
    return sa, sb, off, tuple(names)


@functools.lru_cache(maxsize=None)
def expected(which, **opts):
    sa, sb, off = parity_batch() if which == 'parity' else planted_batch()[:3]
    return pair_linkage(sa, sb, off, **opts)


# ---- the statistic of many pairs of one length at once (the simulations): the same roots by 60 halvings of their brackets
def stat_batch(SA, SB):
    """stat of every pair of the (npairs, n) arrays SA, SB of valid scores (0 for a DEGENERATE pair)"""
    WA, WB = F.signed_t(SA), F.signed_t(SB)

    def halve(S_of, lo, hi):                               # S decreases; S(lo) > 0 > S(hi) wherever the root is interior
        lo, hi = lo.copy(), hi.copy()
        for _ in range(60):
            mid = lo + 0.5 * (hi - lo)
            right = S_of(mid) > 0.0
            lo, hi = np.where(right, mid, lo), np.where(right, hi, mid)
        return lo + 0.5 * (hi - lo)

    def margin(W):
        S_of = lambda p: signed_u(W, p[:, None]).sum(axis=1)
        zero, one = np.zeros(len(W)), np.ones(len(W))
        with np.errstate(divide='ignore', invalid='ignore'):
            at0, at1 = S_of(zero) <= 0.0, S_of(one) >= 0.0
        return np.where(at0, 0.0, np.where(at1, 1.0, halve(S_of, zero, one)))
    pa, pb = margin(WA), margin(WB)
    deg = (pa == 0.0) | (pa == 1.0) | (pb == 0.0) | (pb == 1.0)
    pa_, pb_ = np.where(deg, 0.5, pa), np.where(deg, 0.5, pb)
    V = signed_u(WA, pa_[:, None]) * signed_u(WB, pb_[:, None])
    d_min, d_max = -np.minimum(pa_ * pb_, (1 - pa_) * (1 - pb_)), np.minimum(pa_ * (1 - pb_), (1 - pa_) * pb_)

    def S_of(d):
        with np.errstate(divide='ignore', invalid='ignore'):
            return (V / (1.0 + np.maximum(d[:, None] * V, -1.0))).sum(axis=1)
    at_min = S_of(d_min) <= 0.0
    at_max = ~at_min & (S_of(d_max) >= 0.0)
    d = np.where(at_min, d_min, np.where(at_max, d_max, halve(S_of, d_min, d_max)))
    with np.errstate(divide='ignore', invalid='ignore'):
        g = np.log1p(np.maximum(d[:, None] * V, -1.0)).sum(axis=1)
    return np.where(deg, 0.0, np.maximum(2.0 * g, 0.0))


def null_share(n, sep, pa, pb, seed, N=4000, d=0.0):
    """the share of N seeded pairs of n reads with p_indep <= 0.05 (stat beyond the 0.95 quantile of chi2_1)"""
    rng = np.random.default_rng(seed)
    pairs = [simulate_pair(rng, n, sep, pa, pb, d) for _ in range(N)]
    stat = stat_batch(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    return float((stat > F.CI_DROP_95).mean())
