"""nmod_read_calls / nmod_site_calls (K12) restated in numpy and scipy.special from the text of include/nanomod_hip.h, the mpmath values
the restatement is pinned against, a numpy pivot for the chain, and the seeded inputs the CPU and GPU tests share.  Nothing here calls
the library.  The event codes are rescale_ref's (K11's definition, word for word)."""
import functools

import numpy as np
from scipy import special

import rescale_ref as R

TOO_LARGE = 16
MAX_DEEP = R.MAX_DEEP
WAVE_MAX = 2048                                   # NMOD_CALLS_WAVE_MAX
MAX_NB = 64
DBL_MIN = 2.2250738585072014e-308
INV_SQRT2 = 0.70710678118654752

PIN_Z = (0.0, 1e-3, 1.0, 8.0, 30.0, 38.0, 40.0, 60.0)
PIN_W = (1, 5, 129)
PIN_GATE = 1e-11                                  # two decades under the library's p-value gate of 1e-9


def clamp_p(p):
    return np.where(p < DBL_MIN, DBL_MIN, p)      # NaN passes through


def tails(z):
    """(p, l) of eligible events: p = max(erfc(u), DBL_MIN), l = log(erfcx(u)) - u u, u = |z| 0.70710678118654752"""
    u = np.abs(np.asarray(z, np.float64)) * INV_SQRT2
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        return clamp_p(special.erfc(u)), np.log(special.erfcx(u)) - u * u


def chi2_sf_even(X, W):
    """chi2.sf(X, 2 W) = Q(W, X / 2), the regularised upper incomplete gamma function (the closed sum of the header in exact arithmetic)"""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    with np.errstate(invalid='ignore'):
        return special.gammaincc(np.maximum(W, 1.0), 0.5 * np.maximum(X, 0.0))


def score_read(x, codes, mean, sd, nb):
    """one read: z, p, p_win (NaN where ineligible), and W (0 where ineligible)"""
    n = len(x)
    c = np.where(codes >= 0, codes, 0)
    mu, s = np.asarray(mean, np.float64)[c], np.asarray(sd, np.float64)[c]
    with np.errstate(invalid='ignore'):
        elig = (codes >= 0) & np.isfinite(mu) & np.isfinite(s) & (s > 0.0) & np.isfinite(x)
    z = np.full(n, np.nan)
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        z[elig] = (x[elig] - mu[elig]) / s[elig]
    p, l = np.full(n, np.nan), np.zeros(n)
    p[elig], l[elig] = tails(z[elig])
    if nb == 0:
        return z, p, p.copy(), elig.astype(np.int64)
    W, S = np.zeros(n, np.int64), np.zeros(n)
    for d in range(-nb, nb + 1):                   # the terms in ascending i = j + d; an event that takes no part adds an exact 0
        lo, hi = max(0, -d), min(n, n - d)
        if lo >= hi:
            continue
        part = elig[lo + d:hi + d]
        W[lo:hi] += part
        with np.errstate(invalid='ignore'):
            S[lo:hi] = S[lo:hi] + np.where(part, l[lo + d:hi + d], 0.0)
    P = np.full(n, np.nan)
    with np.errstate(invalid='ignore'):
        P[elig] = clamp_p(chi2_sf_even(-2.0 * S[elig], W[elig]))
    return z, p, P, np.where(elig, W, 0)


def read_calls(val, off, base, k, center, mean, sd, nb=2, alpha=0.01):
    """the whole entry on host arrays: dict(z, p, p_win, W, n_sites, n_called, status) and alpha_margin, the smallest |P / alpha - 1|"""
    val, off = np.asarray(val), np.asarray(off, np.int64)
    nreads = len(off) - 1
    bb = R.as_bytes(base)
    out = dict(z=np.full(len(val), np.nan), p=np.full(len(val), np.nan), p_win=np.full(len(val), np.nan), W=np.zeros(len(val), np.int64),
               n_sites=np.zeros(nreads, np.int32), n_called=np.zeros(nreads, np.int32), status=np.zeros(nreads, np.uint8), alpha_margin=np.inf)
    for i in range(nreads):
        b0, e0 = int(off[i]), int(off[i + 1])
        if e0 - b0 > MAX_DEEP:
            out['status'][i] = TOO_LARGE
            continue
        z, p, P, W = score_read(R.to_double(val[b0:e0]), R.read_codes(bb[b0:e0], k, center), mean, sd, nb)
        out['z'][b0:e0], out['p'][b0:e0], out['p_win'][b0:e0], out['W'][b0:e0] = z, p, P, W
        ok = ~np.isnan(P)
        out['n_sites'][i] = int(ok.sum())
        out['n_called'][i] = int((P[ok] <= alpha).sum())
        if ok.any():
            out['alpha_margin'] = min(out['alpha_margin'], float(np.abs(P[ok] / alpha - 1.0).min()))
    return out


def site_calls(score, off, alpha=0.01):
    score, off = np.asarray(score, np.float64), np.asarray(off, np.int64)
    npos = len(off) - 1
    n_valid, n_called, frac = np.zeros(npos, np.int32), np.zeros(npos, np.int32), np.full(npos, np.nan)
    for i in range(npos):
        s = score[off[i]:off[i + 1]]
        with np.errstate(invalid='ignore'):
            ok = (s >= 0.0) & (s <= 1.0)
            n_valid[i], n_called[i] = int(ok.sum()), int((ok & (s <= alpha)).sum())
        if n_valid[i]:
            frac[i] = np.float64(n_called[i]) / np.float64(n_valid[i])
    return dict(n_valid=n_valid, n_called=n_called, frac=frac)


def pivot(reads, track):
    """the events of a read-level set grouped by position as nmod_pivot_reads does: rows in the reference's order (sorted chromosome, '+'
    before '-', ascending position), the values of a row in read order.  dict(chrom, strand, pos, off, val)"""
    off = np.asarray(reads['off'], np.int64)
    n = np.diff(off)
    nreads = len(n)
    names = np.unique(np.asarray(reads['chrom']).astype(str))
    cid = np.searchsorted(names, np.asarray(reads['chrom']).astype(str))
    minus = np.asarray(reads['strand']).astype(str) == '-'
    rid = np.repeat(np.arange(nreads), n)
    i = np.arange(off[-1]) - off[rid]
    start = np.asarray(reads['start'], np.int64)
    pos = np.where(minus[rid], start[rid] + n[rid] - 1 - i, start[rid] + i)
    key = ((2 * cid[rid] + minus[rid]).astype(np.int64) << 40) | pos
    order = np.argsort(key, kind='stable')                       # stable: read order inside a position
    ukey, first = np.unique(key[order], return_index=True)
    return dict(chrom=names[ukey >> 41], strand=np.where((ukey >> 40) & 1, '-', '+'), pos=ukey & ((1 << 40) - 1),
                off=np.append(first, len(order)).astype(np.int64), val=np.asarray(track)[order])


# --------------------------------------------------------------------------------------------------------------------- mpmath pins

def mp_tails(z):
    """(p, l) of one double z in 50 digits, from the double u the definition forms"""
    import mpmath as mp
    mp.mp.dps = 50
    u = mp.mpf(float(np.abs(np.float64(z)) * INV_SQRT2))
    p = mp.erfc(u)
    return p, mp.log(p)


def mp_window(zs):
    """P of a window of eligible events with the scores zs, unclamped, in 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    x = -sum(mp_tails(z)[1] for z in zs)                          # X / 2
    return mp.gammainc(len(zs), x, mp.inf, regularized=True)


def pin_windows():
    """the windows of the pins: every W of PIN_W filled with every |z| of PIN_Z, one mixed window per W, and windows of zeros around one
    event beyond the clamp of p (the unclamped l keeps such a window above DBL_MIN)"""
    out = [(W, [z] * W) for W in PIN_W for z in PIN_Z]
    cyc = [0.3, -2.5, 8.0, -1e-3, 5.0, 12.0, 0.0, -4.0]
    out += [(W, [cyc[i % len(cyc)] for i in range(W)]) for W in PIN_W]
    return out + [(2 * h + 1, [0.0] * h + [z] + [0.0] * h) for h, z in ((2, 38.0), (2, -39.0), (64, 38.0), (64, -39.0), (64, 60.0))]


def restated_window(zs):
    """the restatement's P of a read that is exactly this window (nb = W: every event sees all of it), at its middle event"""
    W = len(zs)
    z = np.asarray(zs, np.float64)
    _, _, P, Wj = score_read(z, np.zeros(W, np.int64), np.zeros(1), np.ones(1), W)
    assert (Wj == W).all()
    return float(P[W // 2])


def pin_agreement():
    """worst relative deviation of the restatement from mpmath over the pins where mpmath's value is above DBL_MIN: (p, p_win); raises
    where the restatement does not clamp exactly where mpmath's value lies below DBL_MIN"""
    worst_p = worst_w = 0.0
    for z in PIN_Z:
        for s in (z, -z):
            p_mp, l_mp = mp_tails(s)
            p, l = tails(np.array([s]))
            if p_mp >= DBL_MIN:
                worst_p = max(worst_p, abs(float(p[0] / p_mp - 1)))
            else:
                assert p[0] == DBL_MIN, (s, p[0])
            worst_p = max(worst_p, abs(float((l[0] - l_mp) / l_mp)) if l_mp != 0 else abs(float(l[0])))
    for W, zs in pin_windows():
        P_mp = mp_window(zs)
        P = restated_window(zs)
        if P_mp >= DBL_MIN:
            worst_w = max(worst_w, abs(float(P / P_mp - 1)))
        else:
            assert P == DBL_MIN, (W, zs[0], P)
    return worst_p, worst_w


# ------------------------------------------------------------------------------------------------------------------ shared inputs

PARITY_SEED = 31
PARITY_ALPHA = 0.01
PARITY_KC = ((1, 0), (3, 1), (5, 2), (6, 2))
PARITY_NB = (0, 1, 2, 64)
PARITY_DTYPES = ('int16', 'float32', 'float64')


def parity_lengths(k, nb):
    return [0, 1, k - 1, k, 2 * nb, 2 * nb + 1, 63, 64, 65, 511, 512, 513, WAVE_MAX, WAVE_MAX + 1, 5000, 70000]


@functools.lru_cache(maxsize=None)
def parity_inputs(k, center, nb, dtype):
    """the parity read set: dict(val, off, base, mean, sd) — every length at which the code takes another path, model holes (k >= 2),
    contaminated values (so |z| runs far into the clamped tail) and an 'N' in some reads"""
    rng = np.random.default_rng(PARITY_SEED + 1000 * k + 100 * center + nb)
    mean, sd = R.make_model(k)
    vals, bases = [], []
    for i, n in enumerate(parity_lengths(k, nb)):
        b, x = R.draw_read(rng, n, k, center, mean, sd, 0.0, 1.0, n_letters=2 if i % 3 == 0 else 0)
        vals.append(x); bases.append(b)
    lens = [len(v) for v in vals]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    val = R.cast(np.concatenate(vals), dtype)
    for a in (val, off, mean, sd):
        a.setflags(write=False)
    return dict(val=val, off=off, base=np.concatenate(bases), mean=mean, sd=sd)


@functools.lru_cache(maxsize=None)
def parity_expected(k, center, nb, dtype):
    p = parity_inputs(k, center, nb, dtype)
    return read_calls(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], nb, PARITY_ALPHA)


PARITY_CASES = [(k, c, nb, dt) for (k, c) in PARITY_KC for nb in PARITY_NB for dt in PARITY_DTYPES]

DEEP_Z = (0.0, 5.0, 20.0, 37.0, 39.0, 60.0)
DEEP_RUN = 200                                    # events per |z|: longer than the widest window (129)
DEEP_SINGLES = ((150, 38.0), (400, -39.0))        # lone deep events inside the (tripled) run of zeros, more than 128 events from each
                                                  # other and from the run's ends: every window that holds one is zeros but for it


def deep_tail_read():
    """one float64 read over a 1-mer model (mean 0, sd 1), so that x is z: a run of 3 DEEP_RUN zeros that holds the lone events of
    DEEP_SINGLES — their p is clamped, the windows around them are not — then runs of DEEP_RUN events at each further |z| of DEEP_Z, the
    sign alternating"""
    sign = np.where(np.arange(DEEP_RUN) % 2, -1.0, 1.0)
    z = np.concatenate([np.zeros(3 * DEEP_RUN)] + [v * sign for v in DEEP_Z[1:]])
    for j, v in DEEP_SINGLES:
        z[j] = v
    return dict(val=z, off=np.array([0, len(z)], np.int64), base=np.full(len(z), ord('A'), np.uint8), mean=np.zeros(4), sd=np.ones(4))


CHAIN_NB = (0, 2)                                 # the window widths of the chain test


def chain_inputs(seed=77, n_reads=200, genome_len=700, shift_sd=4.0):
    """~200 reads of 300 .. 600 events drawn from a 3-mer model over one short reference, both strands; half of the reads of each strand
    carry a level shift of 4 sd at one position.  (reads, model, planted position)"""
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    planted = genome_len // 2
    chrom, strand, start, vals, bases = [], [], [], [], []
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(300, 601))
        s0 = int(rng.integers(max(0, planted - n + 20), min(genome_len - n, planted - 20) + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        x = mean[codes.clip(0)] + sd[codes.clip(0)] * rng.normal(size=n)
        if (r // 2) % 2 == 0:
            j = int(np.flatnonzero(pos == planted)[0])
            x[j] += shift_sd * sd[codes[j]]
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint(x * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    model = dict(k=k, center=center, mean=mean, sd=sd, n_positions=np.ones(4 ** k, np.int64))
    return reads, model, planted
