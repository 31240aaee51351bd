"""The definition nmod_fdr_adjust is held to: scipy.stats.false_discovery_control on the valid elements (0 <= p <= 1) of a
track, NaN for every other element — as a numpy restatement (fdr_ref) and through scipy itself (fdr_scipy)."""
import numpy as np

ALPHAS = (0.05, 0.04, 0.06, 0.03, 0.07)           # BY: the first level no reference q lies within 1e-12 relative of


def valid_mask(p):
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return (p >= 0.0) & (p <= 1.0)


def fdr_ref(p, method='bh'):
    p = np.asarray(p, dtype=np.float64)
    ok = valid_mask(p)
    q = np.full(p.shape, np.nan)
    ps = p[ok]
    m = ps.size
    if m > 1:
        order = np.argsort(ps, kind='stable')
        i = np.arange(1, m + 1)
        a = ps[order] * (m / i)
        if method == 'by':
            a = a * np.sum(1.0 / i)
        a = np.minimum.accumulate(a[::-1])[::-1]
        ps = np.empty(m)
        ps[order] = np.clip(a, 0.0, 1.0)
    q[ok] = ps
    return q


def fdr_scipy(p, method='bh'):
    from scipy.stats import false_discovery_control
    p = np.asarray(p, dtype=np.float64)
    ok = valid_mask(p)
    q = np.full(p.shape, np.nan)
    ps = p[ok]
    q[ok] = false_discovery_control(np.abs(ps), method=method) if ps.size > 1 else ps        # (abs: -0.0 is 0.0)
    return q


def summary_ref(p, q, alpha):
    p = np.asarray(p, dtype=np.float64)
    ok = valid_mask(p)
    with np.errstate(invalid='ignore'):
        rej = ok & (q <= alpha)
    return dict(tested=int(ok.sum()), excluded=int(p.size - ok.sum()), rejected=int(rej.sum()),
                p_crit=float(np.abs(p[rej]).max()) if rej.any() else float('nan'))


def pick_alpha(q_ref):
    """the first of ALPHAS that no finite reference q is within 1e-12 relative of (asserted on the reference alone)"""
    qf = q_ref[np.isfinite(q_ref)]
    for alpha in ALPHAS:
        if not np.any(np.abs(qf - alpha) <= 1e-12 * alpha):
            return alpha
    raise AssertionError('every level of ALPHAS has a reference q within 1e-12 of it')


def same_summary(got, exp):
    assert got['tested'] == exp['tested'] and got['excluded'] == exp['excluded'] and got['rejected'] == exp['rejected'], (got, exp)
    assert (np.isnan(got['p_crit']) and np.isnan(exp['p_crit'])) or got['p_crit'] == exp['p_crit'], (got, exp)


def check_q(got, ref, method, what=''):
    """BH: equal, NaN in the same places; BY: |q - q_ref| <= 1e-14 q_ref"""
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN pattern differs' % what
    g, r = got[~nan], ref[~nan]
    if method == 'bh':
        bad = g != r
        assert not bad.any(), '%s: %d of %d q differ, first at %d: %r != %r' % (
            what, bad.sum(), bad.size, int(np.argmax(bad)), g[np.argmax(bad)], r[np.argmax(bad)])
    else:
        err = np.abs(g - r)
        bad = err > 1e-14 * r
        assert not bad.any(), '%s: %d of %d q beyond 1e-14, worst rel %g' % (what, bad.sum(), bad.size, (err[bad] / r[bad]).max())
