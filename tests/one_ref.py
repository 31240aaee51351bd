"""The definition of nmod_one_sample (include/nanomod_hip.h, K9) restated in numpy, with scipy's tail functions
(scipy.special.kolmogorov, scipy.stats.t.sf), and the seeded rows the CPU and GPU tests share.  Written from the header's text;
the reference has no such step.

Per position: samples x (as doubles), reference mu, sd (ddof = 0) and optionally its coverage nr.
  m = mean(x), s2 = var(x) (ddof 0), shift = (m - mu) / sd
  F_k = 0.5 erfc(-(x_(k) - mu) / (sd sqrt 2)), D = max_k max(k/n - F_k, F_k - (k-1)/n), ks_p = kolmogorov((sqrt n + 0.12 + 0.11/sqrt n) D)
  t: Welch from the statistics with nr, else the one-sample t; NaN (T_NAN) when its standard error is 0 or n == 1."""
import sys

import numpy as np
from scipy import special, stats

T_NAN, EMPTY, TOO_LARGE, NONFINITE, BAD_REFERENCE = 2, 4, 8, 16, 32
MAX_ONE, MAX_ONE_F64 = 16384, 8192
FIELDS = ('ks_d', 'ks_p', 't_t', 't_p', 'shift', 'mean', 'std')
DBL_MIN, DBL_MAX = sys.float_info.min, sys.float_info.max


def ks_d(x, mu, sd):
    xs = np.sort(np.asarray(x, dtype=np.float64))
    n = len(xs)
    f = 0.5 * special.erfc(-(xs - mu) / (sd * np.sqrt(2.0)))
    k = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(k / n - f), np.max(f - (k - 1.0) / n)))


def ks_p(d, n):
    en = np.sqrt(float(n))
    return float(special.kolmogorov((en + 0.12 + 0.11 / en) * d))


def t_pair(m, s2, n, mu, sd, nr=None):
    """(t, p) of the definition; (nan, nan) where it says so"""
    nan = float('nan')
    if n < 2:
        return nan, nan
    vx = s2 * n / (n - 1.0)
    if nr is None:
        if not vx > 0.0:
            return nan, nan
        t, df = (m - mu) / np.sqrt(vx / n), n - 1.0
    else:
        vr = sd * sd * nr / (nr - 1.0)
        se2 = vx / n + vr / nr
        if not se2 > 0.0:
            return nan, nan
        t = (m - mu) / np.sqrt(se2)
        df = se2 * se2 / ((vx / n) ** 2 / (n - 1.0) + (vr / nr) ** 2 / (nr - 1.0))
    return float(t), float(2.0 * stats.t.sf(abs(t), df))


def position(x, mu, sd, nr=None, cap=MAX_ONE):
    """one position: dict of FIELDS + status"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    nan = float('nan')
    out = {k: nan for k in FIELDS}
    st = 0
    if n == 0:
        st |= EMPTY
    if n > cap:
        st |= TOO_LARGE
    if not np.isfinite(mu) or not np.isfinite(sd) or not sd > 0.0 or (nr is not None and nr < 2):
        st |= BAD_REFERENCE
    if st == 0 and not np.all(np.isfinite(x)):
        st |= NONFINITE
    if st:
        out['status'] = st
        return out
    m, s2 = float(np.mean(x)), float(np.var(x))
    d = ks_d(x, mu, sd)
    p = ks_p(d, n)
    t, tp = t_pair(m, s2, n, mu, sd, nr)
    out.update(ks_d=min(d, DBL_MAX), ks_p=max(p, DBL_MIN), t_t=t if t != t else min(t, DBL_MAX), t_p=tp if tp != tp else max(tp, DBL_MIN),
               shift=(m - mu) / sd, mean=m, std=float(np.sqrt(s2)), status=T_NAN if tp != tp else 0)
    return out


def batch(rows, mu, sd, nr=None, cap=MAX_ONE):
    """rows: per position an array of doubles; returns dict of float64 arrays (FIELDS) and uint8 status"""
    res = [position(r, float(mu[i]), float(sd[i]), None if nr is None else int(nr[i]), cap) for i, r in enumerate(rows)]
    out = {k: np.array([r[k] for r in res], dtype=np.float64) for k in FIELDS}
    out['status'] = np.array([r['status'] for r in res], dtype=np.uint8)
    return out


def csr(rows):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    sig = np.concatenate([np.asarray(r) for r in rows]) if rows and off[-1] else np.zeros(0, dtype=np.asarray(rows[0]).dtype if rows else np.float64)
    return np.ascontiguousarray(sig), off


def grid_rows(rng, sizes, shift_of=None):
    """Rows on the 3-decimal grid as int16 milli-units: spread 0.2 around a level in +-3, so most samples tie; per row the
    reference (mu, sd, nr): sd drawn from 0.1 .. 0.4, mu = level - shift with shift 0 for even rows and 0.3 for odd ones (or
    shift_of(i)), nr from 5 .. 400."""
    rows, mu, sd, nr = [], [], [], []
    for i, n in enumerate(sizes):
        level = int(rng.integers(-3000, 3001))
        rows.append(np.clip(np.rint(level + 200.0 * rng.standard_normal(n)), -32767, 32767).astype(np.int16))
        shift = (0.0 if i % 2 == 0 else 0.3) if shift_of is None else shift_of(i)
        mu.append(level / 1000.0 - shift)
        sd.append(float(rng.uniform(0.1, 0.4)))
        nr.append(int(rng.integers(5, 401)))
    return rows, np.array(mu), np.array(sd), np.array(nr, dtype=np.int32)


def as_dtype(rows, dtype):
    """int16 milli-unit rows in the dtype under test: int16, the doubles k / 1000.0, or their float32 images"""
    if dtype == 'i16':
        return [np.asarray(r, np.int16) for r in rows]
    if dtype == 'f64':
        return [np.asarray(r, np.float64) / 1000.0 for r in rows]
    return [(np.asarray(r, np.float64) / 1000.0).astype(np.float32) for r in rows]


def as_doubles(rows):
    """what the device sees of rows in any dtype"""
    return [np.asarray(r, np.float64) / 1000.0 if np.asarray(r).dtype == np.int16 else np.asarray(r, np.float64) for r in rows]
