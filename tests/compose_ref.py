"""nmod_site_compose (K26) restated in numpy from the text of include/nanomod_hip.h: the open states, the valid and partial reads, the
weights, EM on the simplex from the uniform start with its stop test, the last evaluation, the per-state refits and their boundary
p-values, the responsibilities.  Nothing here calls the library.

The restatement runs the header's operations in the header's order per read; only the order of the sums over the reads differs from
the device's (numpy's pairwise sums here, lane chains and tree reductions there), so the two walk the same EM path to rounding and
stop after the same number of iterations unless a step lands within rounding of tol.  The GPU tests compare at the gates of the
project's other EM with a stop test (tests/test_mix_gpu.py): pi 1e-9 relative, ll 1e-9 relative + 1e-9 absolute, resp 2^-23."""
import math

import numpy as np

MULTI_MAX = 4
TOO_FEW, NO_STATE, NOT_CONVERGED, DEGENERATE, TOO_LARGE = 1, 2, 4, 8, 32
MAX_ITER = 2000
MAX_DEEP = (1 << 24) - 1
SMALL, WAVE = 256, 1024
STAGE_WORDS = 7680                    # site_compose.hip: kCoStageWords, doubles of weights the workgroup form keeps in LDS
DBL_MIN = 2.2250738585072014e-308
DEFAULTS = dict(min_valid=3, max_iter=500, tol=1e-9)

GATE_PI = 1e-9                        # relative
GATE_LL = (1e-9, 1e-9)                # relative, absolute
GATE_RESP = 2.0 ** -23                # absolute
ITERS_NEAR_TOL = 1e-6                 # iters may differ where the restatement's last step lies within this share of tol of tol


def stage_reads(n_alt):
    return STAGE_WORDS // (n_alt + 1)


def classify(S):
    """S: n_alt x n scores of one row.  (open mask over the states, valid reads, partial reads)"""
    with np.errstate(invalid='ignore'):
        fin = np.abs(S) <= np.finfo(np.float64).max
    open_ = fin.any(axis=1)
    if not open_.any():
        return open_, np.zeros(S.shape[1], bool), np.zeros(S.shape[1], bool)
    valid = fin[open_].all(axis=0)
    partial = fin.any(axis=0) & ~valid
    return open_, valid, partial


def weights(S, open_, valid):
    """(W: (n_alt + 1) x n_valid, mx: n_valid) of the valid reads"""
    Sv = S[:, valid]
    n_alt = S.shape[0]
    mx = np.zeros(Sv.shape[1])
    for m in range(n_alt):
        if open_[m]:
            mx = np.where(Sv[m] > mx, Sv[m], mx)
    W = np.zeros((n_alt + 1, Sv.shape[1]))
    with np.errstate(over='ignore', invalid='ignore'):
        W[0] = np.exp(-mx)
        for m in range(n_alt):
            if open_[m]:
                W[m + 1] = np.exp(Sv[m] - mx)
    return W, mx


def _den(pi, W):
    t = pi[:, None] * W
    den = t[0].copy()
    for m in range(1, len(pi)):
        den = den + t[m]
    return t, den


def fit(W, mx, active, max_iter, tol):
    """EM over the states of `active` (a bool per state, canonical first): dict(pi, ll, iters, nc, degen, last_step)"""
    nv = float(W.shape[1])
    pi = np.where(active, 1.0 / float(active.sum()), 0.0)
    iters, done, degen, step = 0, False, False, np.inf
    for _ in range(max_iter):
        t, den = _den(pi, W)
        if not (den > 0.0).all():
            degen = True
            break
        q = 1.0 / den
        R = (t * q).sum(axis=1)
        new = R / nv
        step = float(np.abs(new - pi).max())
        pi = new
        iters += 1
        if tol > 0.0 and step <= tol:
            done = True
            break
    t, den = _den(pi, W)
    if not (den > 0.0).all():
        degen = True
    with np.errstate(divide='ignore'):
        ll = float((np.log(den) + mx).sum()) if not degen else np.nan
    return dict(pi=pi, ll=ll, iters=iters, nc=not done and not degen, degen=degen, last_step=step, t=t, den=den)


def p_boundary(stat):
    return 1.0 if stat == 0.0 else max(0.5 * math.erfc(math.sqrt(stat / 2.0)), DBL_MIN)


def row(S, min_valid=3, max_iter=500, tol=1e-9, test=True, states=None):
    """one row: S is n_alt x n.  dict(pi, ll, stat, stat_m, p_m, n_valid, n_partial, iters, open_mask, status, resp, last_step (of the
    main fit), near_tol: whether a fit's last step lies within ITERS_NEAR_TOL * tol of tol).  states: the states to test (default: all)"""
    S = np.asarray(S, np.float64)
    n_alt, n = S.shape
    nan = np.nan
    out = dict(pi=np.full(n_alt + 1, nan), ll=nan, stat=nan, stat_m=np.full(n_alt, nan), p_m=np.full(n_alt, nan), n_valid=0, n_partial=0,
               iters=0, open_mask=0, status=0, resp=np.full((n_alt + 1, n), nan), last_step=nan, near_tol=False)
    if n > MAX_DEEP:
        out['status'] = TOO_LARGE
        return out
    open_, valid, partial = classify(S)
    out['n_valid'], out['n_partial'] = int(valid.sum()), int(partial.sum())
    out['open_mask'] = int(sum(1 << m for m in range(n_alt) if open_[m]))
    if not open_.any():
        out['status'] = NO_STATE
        return out
    if out['n_valid'] < min_valid:
        out['status'] = TOO_FEW
        return out
    W, mx = weights(S, open_, valid)
    active = np.concatenate([[True], open_])
    f = fit(W, mx, active, max_iter, tol)
    near = lambda g: tol > 0.0 and abs(g['last_step'] - tol) <= ITERS_NEAR_TOL * tol
    out['near_tol'] = near(f)
    if f['degen']:
        out['status'] = DEGENERATE
        return out
    out.update(pi=f['pi'], ll=f['ll'], stat=2.0 * max(f['ll'], 0.0), iters=f['iters'], last_step=f['last_step'])
    status = NOT_CONVERGED if f['nc'] else 0
    out['resp'][:, valid] = f['t'] * (1.0 / f['den'])
    if test:
        for m in range(1, n_alt + 1):
            if not open_[m - 1] or (states is not None and m not in states):
                continue
            act = active.copy()
            act[m] = False
            g = fit(W, mx, act, max_iter, tol)
            out['near_tol'] = out['near_tol'] or near(g)
            if g['nc']:
                status |= NOT_CONVERGED
            if g['degen']:
                status |= DEGENERATE
                continue
            out['stat_m'][m - 1] = 2.0 * max(f['ll'] - g['ll'], 0.0)
            out['p_m'][m - 1] = p_boundary(out['stat_m'][m - 1])
    out['status'] = status
    return out


FIELDS = ('pi', 'll', 'stat', 'stat_m', 'p_m', 'n_valid', 'n_partial', 'iters', 'open_mask', 'status', 'last_step', 'near_tol')


def site_compose(scores, off=None, stride=0, **opts):
    """the whole entry on host arrays: scores a sequence of n_alt vectors; dict of arrays (pi: n_alt + 1 x npos, stat_m, p_m: n_alt x npos,
    resp: n_alt + 1 x scores)"""
    S = np.stack([np.asarray(s, np.float64) for s in scores])
    n_alt, total = S.shape
    if off is None:
        off = np.arange(0, total + 1, stride, dtype=np.int64)
    off = np.asarray(off, np.int64)
    npos = len(off) - 1
    rows = [row(S[:, off[i]:off[i + 1]], **opts) for i in range(npos)]
    out = {}
    for f in FIELDS:
        a = np.array([r[f] for r in rows]) if npos else np.zeros((0,) + np.shape(row(np.zeros((n_alt, 0)))[f]))
        out[f] = a.T.copy() if a.ndim == 2 else a
    out['resp'] = np.full((n_alt + 1, total), np.nan)
    for i, r in enumerate(rows):
        out['resp'][:, off[i]:off[i + 1]] = r['resp']
    for f, dt in (('n_valid', np.int32), ('n_partial', np.int32), ('iters', np.int32), ('open_mask', np.uint8), ('status', np.uint8)):
        out[f] = out[f].astype(dt)
    return out


# -------------------------------------------------------------------------------------------- equal-length rows, all at once (the null
# simulation: thousands of rows through the same operations, the rows that have stopped left out of the later iterations)

def fit_batch(W, mx, active, max_iter, tol):
    """fit over rows of one length: W rows x (n_alt + 1) x n, mx rows x n, every read valid; active: a bool per state.  (pi, ll, iters, nc)"""
    rows, ns, n = W.shape
    pi = np.tile(np.where(active, 1.0 / float(active.sum()), 0.0), (rows, 1))
    iters = np.zeros(rows, np.int64)
    live = np.arange(rows)
    for _ in range(max_iter):
        if not len(live):
            break
        Wl = W[live]
        t = pi[live][:, :, None] * Wl
        den = t[:, 0].copy()
        for m in range(1, ns):
            den = den + t[:, m]
        assert (den > 0.0).all()
        new = (t * (1.0 / den)[:, None, :]).sum(axis=2) / float(n)
        step = np.abs(new - pi[live]).max(axis=1)
        pi[live] = new
        iters[live] += 1
        live = live[~((tol > 0.0) & (step <= tol))]
    t = pi[:, :, None] * W
    den = t[:, 0].copy()
    for m in range(1, ns):
        den = den + t[:, m]
    ll = (np.log(den) + mx).sum(axis=1)
    nc = np.zeros(rows, bool)
    nc[live] = True
    return pi, ll, iters, nc


def test_state_batch(S, m, max_iter=MAX_ITER, tol=1e-8):
    """rows x n_alt x n finite scores: (pi, stat_m, p_m, not converged) of the test of state m (1-based) per row"""
    S = np.asarray(S, np.float64)
    rows, n_alt, n = S.shape
    mx = np.maximum(S.max(axis=1), 0.0)
    W = np.concatenate([np.exp(-mx)[:, None, :], np.exp(S - mx[:, None, :])], axis=1)
    full = np.ones(n_alt + 1, bool)
    pi, ll, _, nc = fit_batch(W, mx, full, max_iter, tol)
    without = full.copy()
    without[m] = False
    _, ll0, _, nc0 = fit_batch(W, mx, without, max_iter, tol)
    stat = 2.0 * np.maximum(ll - ll0, 0.0)
    p = np.array([p_boundary(float(s)) for s in stat])
    return pi, stat, p, nc | nc0


test_state_batch.__test__ = False     # (not a test: pytest collects by name)


def simulate_rows(rng, rows, n, shares, sep=2.0):
    """rows x n reads whose state is drawn with the given shares (canonical first; len(shares) - 1 = n_alt), observed through one unit
    normal coordinate per state, state m's level at sep on its own coordinate: s_im = sep y_im - sep^2 / 2, the exact log-likelihood
    ratio of state m against canonical.  rows x n_alt x n"""
    shares = np.asarray(shares, np.float64)
    n_alt = len(shares) - 1
    z = rng.choice(len(shares), size=(rows, n), p=shares)
    y = rng.normal(size=(rows, n_alt, n))
    for m in range(1, n_alt + 1):
        y[:, m - 1, :] += sep * (z == m)
    return sep * y - 0.5 * sep * sep


# ------------------------------------------------------------------------------------------------------------------ shared inputs
PARITY_OPTS = dict(min_valid=3, max_iter=400, tol=1e-8)


def parity_lengths(n_alt):
    """rows of 1, 2, 3 reads (TOO_FEW below min_valid), around the class steps, and one row past the LDS-resident limit of the workgroup class"""
    return [1, 2, 3, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, stage_reads(n_alt) + 1]


def parity_batch(n_alt, seed=0):
    """(scores: n_alt vectors, off) — per length four rows: every state present at shares 0.5 / n_alt; the last state closed (all NaN) and
    some reads partial (a NaN, +inf or -inf in one open state); state 1 absent with a canonical majority (its share is driven to the
    boundary); and a row with |s| = 700 in both directions.  Then a row of all-zero scores, an all-NaN row (NO_STATE), an empty row"""
    rng = np.random.default_rng(2026 + 10 * n_alt + seed)
    rows = []
    for n in parity_lengths(n_alt):
        shares = np.array([0.5] + [0.5 / n_alt] * n_alt)
        a = simulate_rows(rng, 1, n, shares, sep=2.5)[0]
        b = simulate_rows(rng, 1, n, shares, sep=2.0)[0]
        b[n_alt - 1] = np.nan                                                # (n_alt = 1: nothing is open)
        bad = rng.random(n) < 0.1
        if n_alt > 1:
            b[0, bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
        c = simulate_rows(rng, 1, n, np.array([0.7, 0.0] + [0.3 / max(n_alt - 1, 1)] * (n_alt - 1)) if n_alt > 1 else np.array([1.0, 0.0]), sep=3.0)[0]
        d = simulate_rows(rng, 1, n, shares, sep=1.5)[0]
        d[:, ::3] = 700.0 * np.sign(d[:, ::3])
        d[0, 1::7] = -700.0
        rows += [a, b, c, d]
    rows += [np.zeros((n_alt, 40)), np.full((n_alt, 9), np.nan), np.zeros((n_alt, 0))]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([r.shape[1] for r in rows])
    S = np.concatenate(rows, axis=1)
    return [np.ascontiguousarray(S[m]) for m in range(n_alt)], off


def stoich_rows(seed=5):
    """well-separated rows for the comparison with K14 at n_alt = 1: (score, off); 8 spreads apart, shares 0.2 / 0.5 / 0.8, 20 .. 2 000 reads"""
    import stoich_ref as SR
    rng = np.random.default_rng(seed)
    rows = [SR.simulate_row(rng, n, 8.0, pi) for n in (20, 200, 300, 1100, 2000) for pi in (0.2, 0.5, 0.8)]
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return np.concatenate(rows), off


STOICH_TOL = 1e-12
STOICH_GATE = 100.0 * STOICH_TOL      # pi absolute, stat relative


def p_gate(stat):
    """p_null = erfc(sqrt(stat / 2)) / 2 falls like exp(-stat / 2): a relative deviation r of stat moves it by about r stat / 2 relative;
    erfc itself within 20 eps"""
    return STOICH_GATE * (0.5 * stat + 1.0) + 20.0 * 2.0 ** -52
