"""The definition of nmod_mix_fraction (include/nanomod_hip.h) restated in numpy, the same in 40-digit mpmath, and the seeded
inputs the CPU conditioning pin and the GPU parity test share.  Written from the header's text; the reference has no such step.

Per position: R the reference group, Y the mixed one, mu = mean(R), s2 = var(R) (ddof 0), s = sqrt(s2), d = mean(Y) - mu;
y ~ (1 - pi) N(mu, s2) + pi N(m, v), v == s2 ('equal', 0) or free and floored at s2 / 16 ('free', 1); start pi = 0.5,
m = mu + 2 d, v = s2."""
import numpy as np

EQUAL, FREE = 0, 1
NOT_CONVERGED, DEGENERATE, SKIPPED, VAR_FLOORED, TOO_LARGE = 1, 2, 4, 8, 16
FIELDS = ('pi', 'mu_mod', 'sd_mod', 'llr')
MODEL_BY_NAME = {'equal': EQUAL, 'free': FREE}


def as_double(a):
    """samples as the doubles the definition sees: float32 up-cast, int16 k / 1000.0, float64 as is"""
    a = np.asarray(a)
    return a.astype(np.float64) / 1000.0 if a.dtype == np.int16 else a.astype(np.float64)


def softplus(x):
    """ln(1 + e^x) without overflow"""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def degenerate_by_input(x, y):
    x, y = as_double(x), as_double(y)
    return len(x) < 2 or len(y) < 2 or not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))) or bool(np.all(x == x[0])) or not np.var(x) > 0.0


def _nan_result(ny):
    r = {k: np.nan for k in FIELDS}
    r.update(iters=0, status=DEGENERATE, resp=np.full(ny, np.nan), delta=np.nan, delta_prev=np.nan)
    return r


def _t(y, mu, s2, pi, m, v, model):
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        t = np.log((1.0 - pi) / pi)
        if model == FREE:
            t = t + 0.5 * np.log(v / s2)
        return t + (y - m) ** 2 / (2.0 * v) - (y - mu) ** 2 / (2.0 * s2)


def _run(x, y, model, max_iter, tol, fixed):
    """`fixed`: run exactly max_iter iterations (no stopping rule); else stop when delta <= tol (tol > 0)"""
    x, y = as_double(x), as_double(y)
    if degenerate_by_input(x, y):
        return _nan_result(len(y))
    mu, s2 = float(np.mean(x)), float(np.var(x))
    s, n = np.sqrt(s2), len(y)
    pi, m, v = 0.5, mu + 2.0 * (float(np.mean(y)) - mu), s2
    delta = delta_prev = np.nan
    floored, iters, converged = False, 0, False
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for k in range(1, max_iter + 1):
            r = 1.0 / (1.0 + np.exp(_t(y, mu, s2, pi, m, v, model)))
            w = float(np.sum(r))
            if not w > 0.0:                                   # every responsibility underflowed
                return _nan_result(n)
            pn, mn, vn, fl = w / n, float(np.sum(r * y)) / w, v, False
            if model == FREE:
                vn = float(np.sum(r * (y - mn) ** 2)) / w
                fl = vn < s2 / 16.0
                vn = max(vn, s2 / 16.0)
            dl = max(abs(pn - pi), abs(mn - m) / s)
            if model == FREE:
                dl = max(dl, abs(np.sqrt(vn) - np.sqrt(v)) / s)
            delta_prev, delta = delta, dl
            pi, m, v, floored, iters = pn, mn, vn, fl, k
            if not fixed and tol > 0.0 and dl <= tol:
                converged = True
                break
        t = _t(y, mu, s2, pi, m, v, model)
        llr = 2.0 * float(np.sum(np.log(1.0 - pi) + softplus(-t)))
        resp = 1.0 / (1.0 + np.exp(t))
    status = (VAR_FLOORED if floored else 0) | (0 if converged or fixed else NOT_CONVERGED)
    return dict(pi=pi, mu_mod=m, sd_mod=float(np.sqrt(v)), llr=llr, iters=iters, status=status, resp=resp, delta=delta,
                delta_prev=delta_prev, s=s)


def em(x, y, model, iters):
    """exactly `iters` iterations of the definition; also `delta` of the last iteration and `delta_prev` of the one before.
    status holds DEGENERATE / VAR_FLOORED only (whether a run converged is the caller's rule: see run)"""
    return _run(x, y, model, int(iters), 0.0, True)


def run(x, y, model, max_iter=200, tol=1e-6):
    """the whole definition with its stopping rule: delta <= tol (tol > 0) or max_iter iterations"""
    return _run(x, y, model, int(max_iter), float(tol), False)


def em_mp(x, y, model, iters, dps=40):
    """em in mpmath at `dps` digits (the inputs are taken as the exact doubles they are); pi, mu_mod, sd_mod, llr as mpf + s"""
    import mpmath as mp
    with mp.workdps(dps):
        x = [mp.mpf(float(u)) for u in as_double(x)]
        y = [mp.mpf(float(u)) for u in as_double(y)]
        n = len(y)
        mu = mp.fsum(x) / len(x)
        s2 = mp.fsum((u - mu) ** 2 for u in x) / len(x)
        pi, m, v = mp.mpf(0.5), mu + 2 * (mp.fsum(y) / n - mu), s2
        a = [(u - mu) ** 2 / (2 * s2) for u in y]

        def tt():
            c = mp.log((1 - pi) / pi) + (mp.log(v / s2) / 2 if model == FREE else 0)
            h = 1 / (2 * v)
            return [c + (u - m) ** 2 * h - ai for u, ai in zip(y, a)]
        for _ in range(int(iters)):
            r = [1 / (1 + mp.exp(t)) for t in tt()]
            w = mp.fsum(r)
            pi, m = w / n, mp.fsum(ri * u for ri, u in zip(r, y)) / w
            if model == FREE:
                v = max(mp.fsum(ri * (u - m) ** 2 for ri, u in zip(r, y)) / w, s2 / 16)
        llr = 2 * mp.fsum(mp.log(1 - pi) + mp.log(1 + mp.exp(-t)) for t in tt())
        return dict(pi=pi, mu_mod=m, sd_mod=mp.sqrt(v), llr=llr, s=mp.sqrt(s2))


# ---------------------------------------------------------------------------------------------------- shared inputs
SMALL, WAVE = 256, 1024          # mix_fraction.hip: kMixSmall / kMixWave, the largest |Y| of the 16-lane and of the whole-wave form
PARITY_SIZES = (2, 3, 5, 15, 16, 17, 40, 100, 200, SMALL - 1, SMALL, SMALL + 1, 400, 700, WAVE - 1, WAVE, WAVE + 1, 1500, 3000)
PARITY_FRACTIONS = (0.0, 0.1, 0.3, 0.5, 0.8, 1.0)


def planted_rows(rng, n_ref, n_mix, frac, shift_sigma, sigma=0.2):
    """one position on the 3-decimal grid as int16 milli-units: a level, the reference group around it, the mixed group with
    round(frac n) of its reads shifted by shift_sigma sigma.  Returns (ref, mix, planted mask of mix)"""
    level = int(rng.integers(-3000, 3001))
    ref = np.rint(level + 1000.0 * sigma * rng.standard_normal(n_ref))
    mix = level + 1000.0 * sigma * rng.standard_normal(n_mix)
    planted = np.zeros(n_mix, dtype=bool)
    planted[rng.permutation(n_mix)[:int(round(frac * n_mix))]] = True
    mix = np.rint(mix + planted * (1000.0 * sigma * shift_sigma))
    return ref.astype(np.int16), mix.astype(np.int16), planted


def parity_inputs(seed=20260917):
    """The positions of the GPU parity test, one per entry of PARITY_SIZES (the size of the MIXED group; every size class of the
    register-resident forms, their edges, and the streaming form), ragged, 3-decimal values, planted fractions 0 .. 1 cycling
    through PARITY_FRACTIONS at 3 .. 5 sigma (fraction 0 = a null position).  Returns (ref_rows, mix_rows) as lists of int16
    arrays; the reference group has an unrelated size in 2 .. 3 000."""
    rng = np.random.default_rng(seed)
    ref_rows, mix_rows = [], []
    for i, ny in enumerate(PARITY_SIZES):
        nr = (2, 3, 3000, 37)[i] if i < 4 else int(rng.integers(20, 600))
        frac = PARITY_FRACTIONS[i % len(PARITY_FRACTIONS)]
        while True:
            r, y, _ = planted_rows(rng, nr, ny, frac, 3.0 + (i % 3))
            if len(np.unique(r)) > 1:                        # (a constant reference group is a degenerate position, tested apart)
                break
        ref_rows.append(r); mix_rows.append(y)
    return ref_rows, mix_rows


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return (np.concatenate(rows) if rows else np.zeros(0, np.int16)), off
