"""nmod_rescale_reads (K11) restated in numpy from the text of include/nanomod_hip.h, an exact-rational fit on the doubles as they
are, and the seeded inputs the CPU and GPU tests share.  Nothing here calls the library."""
import functools
import math
from fractions import Fraction

import numpy as np

FIT_APPLY, FIT_ONLY, APPLY_ONLY = 0, 1, 2
TOO_FEW, DEGENERATE, OUT_OF_RANGE, CLAMPED, TOO_LARGE = 1, 2, 4, 8, 16
MAX_DEEP = 2 ** 24 - 1
WAVE_MAX = 2048                                   # NMOD_RESCALE_WAVE_MAX: a wave up to here, a workgroup beyond

_VAL = np.full(256, -1, np.int64)
_VAL[[ord(c) for c in 'ACGT']] = np.arange(4)


def as_bytes(base):
    b = np.asarray(base)
    return b if b.dtype == np.uint8 else np.ascontiguousarray(b.astype('S1')).view(np.uint8)


def read_codes(base, k, center):
    """code of every event of ONE read from the bytes base[j - center .. j + k - 1 - center]; -1 when the window leaves the read or
    holds a byte other than A, C, G, T"""
    v = _VAL[as_bytes(base)]
    n = len(v)
    code = np.zeros(n, np.int64)
    ok = np.ones(n, bool)
    j = np.arange(n)
    for d in range(-center, k - center):
        p = j + d
        inside = (p >= 0) & (p < n)
        vv = np.where(inside, v[np.clip(p, 0, max(n - 1, 0))] if n else 0, -1)
        ok &= vv >= 0
        code = code * 4 + np.where(vv >= 0, vv, 0)
    return np.where(ok, code, -1)


def to_double(val):
    val = np.asarray(val)
    return val.astype(np.float64) / 1000.0 if val.dtype == np.int16 else val.astype(np.float64)


def fit_read(x, codes, mean, sd, weighted=True, clip_sigma=3.0, clip_rounds=2, min_events=50, scale_lo=0.5, scale_hi=2.0):
    """the fit of one read: dict(shift, scale, n_used, status) and, for the tests' input conditions, clip_margin (the smallest distance
    of an eligible event from a clip boundary over all rounds), kept (the last round's kept set), mu / w (per event)"""
    n = len(x)
    fail = lambda st, used=0, **kw: dict(shift=0.0, scale=1.0, n_used=int(used), status=st, clip_margin=np.inf, **kw)
    if n > MAX_DEEP:
        return fail(TOO_LARGE)
    c = np.where(codes >= 0, codes, 0)
    mu, s = np.asarray(mean, np.float64)[c], np.asarray(sd, np.float64)[c]
    with np.errstate(invalid='ignore'):
        elig = (codes >= 0) & np.isfinite(mu) & np.isfinite(s) & (s > 0.0) & np.isfinite(x)
    if not elig.any():
        return fail(TOO_FEW)
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.where(elig, 1.0 / (s * s) if weighted else 1.0, 0.0)
    j0 = int(np.flatnonzero(elig)[0])
    dm_all, dx_all = mu - mu[j0], x - x[j0]
    a, b, margin = 0.0, 1.0, np.inf
    keep = elig
    for r in range(clip_rounds + 1):
        if r > 0:
            with np.errstate(invalid='ignore'):
                res, lim = np.abs(x - a - b * mu), clip_sigma * abs(b) * s
                keep = elig & (res <= lim)
                margin = min(margin, float(np.abs(res - lim)[elig].min()))
        used = int(keep.sum())
        if used < min_events:
            return dict(fail(TOO_FEW, used), clip_margin=margin)
        wk, dm, dx = w[keep], dm_all[keep], dx_all[keep]
        W = math.fsum(wk)
        mb, xb = math.fsum(wk * dm) / W, math.fsum(wk * dx) / W
        smm, smx = math.fsum(wk * (dm - mb) * (dm - mb)), math.fsum(wk * (dm - mb) * (dx - xb))
        with np.errstate(divide='ignore', invalid='ignore'):
            b_new = np.float64(smx) / np.float64(smm)
        if not smm > 0.0 or not np.isfinite(b_new) or not b_new > 0.0:
            return dict(fail(DEGENERATE, used), clip_margin=margin)
        b = float(b_new)
        a = (x[j0] + xb) - b * (mu[j0] + mb)
        if not np.isfinite(a):
            return dict(fail(DEGENERATE, used), clip_margin=margin)
    if not scale_lo <= b <= scale_hi:
        return dict(fail(OUT_OF_RANGE, used), clip_margin=margin)
    return dict(shift=float(a), scale=b, n_used=used, status=0, clip_margin=margin, kept=keep, mu=mu, w=w)


def apply_read(val, a, b):
    """(rescaled events in val's dtype, clamped, 1000 x' per event (int16 only; NaN where x is not finite))"""
    val = np.asarray(val)
    x = to_double(val)
    fin = np.isfinite(x)
    r = 1.0 / b
    with np.errstate(invalid='ignore', over='ignore'):
        y = (x - a) * r
    if val.dtype == np.float64:
        return np.where(fin, y, x), False, None
    if val.dtype == np.float32:
        with np.errstate(over='ignore'):
            return np.where(fin, y.astype(np.float32), val), False, None
    t = 1000.0 * y
    q = np.rint(t)
    sat = ~(np.abs(q) <= 32767.0)
    return np.where(sat, np.where(q > 0, 32767, -32767), np.where(sat, 0, q)).astype(np.int16), bool(sat.any()), t


def rescale(val, off, base, k=None, center=None, mean=None, sd=None, *, mode=FIT_APPLY, weighted=True, clip_sigma=3.0, clip_rounds=2,
            min_events=50, scale_lo=0.5, scale_hi=2.0, shift=None, scale=None):
    """the whole entry on host arrays: dict(shift, scale, n_used, status, val, clip_margin, t1000 (int16: 1000 x' per event))"""
    val, off = np.asarray(val), np.asarray(off, np.int64)
    nreads = len(off) - 1
    bb = as_bytes(base) if base is not None else None
    out = dict(shift=np.zeros(nreads), scale=np.ones(nreads), n_used=np.zeros(nreads, np.int32), status=np.zeros(nreads, np.uint8),
               val=val.copy(), clip_margin=np.inf, t1000=np.full(len(val), np.nan))
    if mode == APPLY_ONLY:
        out['shift'], out['scale'] = np.array(shift, np.float64), np.array(scale, np.float64)
    for i in range(nreads):
        b0, e0 = int(off[i]), int(off[i + 1])
        v = val[b0:e0]
        if mode == APPLY_ONLY:
            a, b = float(out['shift'][i]), float(out['scale'][i])
            st = TOO_LARGE if len(v) > MAX_DEEP else (0 if (np.isfinite(a) and np.isfinite(b) and b > 0.0) else DEGENERATE)
        else:
            too_large = len(v) > MAX_DEEP                                   # (its codes are never looked at)
            f = fit_read(to_double(v), None if too_large else read_codes(bb[b0:e0], k, center), mean, sd, weighted, clip_sigma, clip_rounds, min_events, scale_lo, scale_hi)
            a, b, st = f['shift'], f['scale'], f['status']
            out['shift'][i], out['scale'][i], out['n_used'][i] = a, b, f['n_used']
            out['clip_margin'] = min(out['clip_margin'], f['clip_margin'])
        if not st and mode != FIT_ONLY:
            y, clamped, t = apply_read(v, a, b)
            out['val'][b0:e0] = y
            if t is not None:
                out['t1000'][b0:e0] = t
            st |= CLAMPED if clamped else 0
        out['status'][i] = st
    if mode == FIT_ONLY:
        del out['val']
    return out


def _scaled_ints(v):
    """the doubles of v as integers times one power of two: (ints, exponent)"""
    v = np.asarray(v, np.float64)
    nz = v[v != 0.0]
    if len(nz) == 0:
        return [0] * len(v), 0
    e = int(np.frexp(nz)[1].min()) - 53
    return [int(math.ldexp(t, -e)) for t in v.tolist()], e


def exact_fit(x, mu, w):
    """weighted least squares of x ~ a + b mu in exact rational arithmetic on the doubles as they are: (a, b) as Fractions"""
    xi, ex = _scaled_ints(x)
    mi, em = _scaled_ints(mu)
    wi, ew = _scaled_ints(w)
    W = sum(wi)
    sm = sum(p * q for p, q in zip(wi, mi))
    sx = sum(p * q for p, q in zip(wi, xi))
    smm = sum(p * q * q for p, q in zip(wi, mi))
    smx = sum(p * q * t for p, q, t in zip(wi, mi, xi))
    # every sum carries 2^ew; sm, smm 2^em per factor of mu; sx, smx 2^ex per factor of x
    Smm = Fraction(smm * W - sm * sm, W)                   # times 2^(ew + 2 em)
    Smx = Fraction(smx * W - sm * sx, W)                   # times 2^(ew + em + ex)
    b = Smx / Smm * Fraction(2) ** (ex - em)
    a = Fraction(sx, W) * Fraction(2) ** ex - b * Fraction(sm, W) * Fraction(2) ** em
    return a, b


# ------------------------------------------------------------------------------------------------------------------ shared inputs

def make_model(k, seed=5, holes=True):
    """a k-mer table: levels N(0, 1), spreads U(0.1, 0.3); with `holes` (k >= 2) one NaN level, one NaN spread, one zero and one
    negative spread"""
    rng = np.random.default_rng(1000 * k + seed)
    m = 4 ** k
    mean, sd = rng.normal(0.0, 1.0, m), rng.uniform(0.1, 0.3, m)
    if holes and k >= 2:
        mean[3], sd[6], sd[9], sd[12] = np.nan, np.nan, 0.0, -0.2
    return mean, sd


def draw_values(rng, base, k, center, mean, sd, a, b, contaminate=True):
    """the events of a read with the bases `base`, drawn from the model at shift a and scale b, on the 3-decimal grid; an event without
    a usable k-mer gets plain noise; contaminate: 5 % of the events + 1 unit, 1 % uniform over +-5"""
    n = len(base)
    codes = read_codes(base, k, center)
    c = np.where(codes >= 0, codes, 0)
    mu, s = mean[c], sd[c]
    good = (codes >= 0) & np.isfinite(mu) & np.isfinite(s) & (s > 0)
    z = rng.normal(size=n)
    x = np.where(good, a + b * (np.where(good, mu, 0.0) + np.where(good, s, 0.0) * z), z)
    if contaminate:
        u = rng.random(n)
        x = np.where(u < 0.05, x + 1.0, x)
        x = np.where(u > 0.99, rng.uniform(-5.0, 5.0, n), x)
    return np.rint(np.clip(x, -30.0, 30.0) * 1000.0) / 1000.0


def draw_read(rng, n, k, center, mean, sd, a, b, contaminate=True, n_letters=0):
    """one read of n events with random bases: (base bytes, values as doubles on the 3-decimal grid)"""
    base = rng.choice(np.frombuffer(b'ACGT', np.uint8), n)
    if n_letters and n > 8:
        base[rng.choice(n, n_letters, replace=False)] = ord('N')
    return base, draw_values(rng, base, k, center, mean, sd, a, b, contaminate)


_COMP = np.arange(256, dtype=np.uint8)
_COMP[[ord(c) for c in 'ACGT']] = [ord(c) for c in 'TGCA']


def make_read_set(seed, k, center, mean, sd, *, chroms=('chr1', 'chr2'), genome_len=300, reads_per_strand=8, full_span=False, planted=True,
                  contaminate=False, n_at=(), dtype='int16'):
    """a read-level set (container.READ_FIELDS) over random genomes: a '+' read's event i lies at start + i and carries the genome's
    base there, a '-' read's at start + n - 1 - i and carries the complement (the read's own base).  full_span: every read covers its
    whole chromosome.  Also a_true / b_true per read and the genomes."""
    rng = np.random.default_rng(seed)
    chrom, strand, start, vals, bases, a_true, b_true, genomes = [], [], [], [], [], [], [], {}
    for ch in chroms:
        genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
        for p in n_at:
            genome[p] = ord('N')
        genomes[ch] = genome
        for sd_ in '+-':
            for _ in range(reads_per_strand):
                s0 = 0 if full_span else int(rng.integers(0, genome_len // 3))
                n = genome_len if full_span else int(rng.integers(genome_len // 2, genome_len - s0 + 1))
                pos = s0 + np.arange(n) if sd_ == '+' else s0 + n - 1 - np.arange(n)
                b = genome[pos] if sd_ == '+' else _COMP[genome[pos]]
                a0, b0 = (rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.25)) if planted else (0.0, 1.0)
                chrom.append(ch); strand.append(sd_); start.append(s0); bases.append(b); a_true.append(a0); b_true.append(b0)
                vals.append(draw_values(rng, b, k, center, mean, sd, a0, b0, contaminate))
    off = np.zeros(len(vals) + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    return dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off, norm_mean=cast(np.concatenate(vals), dtype),
                base=np.concatenate(bases).view('S1'), a_true=np.array(a_true), b_true=np.array(b_true), genomes=genomes)


def cast(x, dtype):
    dtype = np.dtype(dtype)
    return np.rint(x * 1000.0).astype(np.int16) if dtype == np.int16 else x.astype(dtype)


def parity_lengths(k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 300, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 5000, 70000, 37, 1000]


PARITY_MIN_EVENTS = 30
PARITY_SEED = 20


@functools.lru_cache(maxsize=None)
def parity_inputs(k, center, dtype):
    """the parity read set: dict(val, off, base, mean, sd) — every length at which the code takes another path, an 'N' in some reads"""
    rng = np.random.default_rng(PARITY_SEED + 100 * k + 10 * center)
    mean, sd = make_model(k)
    vals, bases = [], []
    for i, n in enumerate(parity_lengths(k)):
        b, x = draw_read(rng, n, k, center, mean, sd, rng.uniform(-0.3, 0.3), rng.uniform(0.8, 1.25), n_letters=2 if i % 3 == 0 else 0)
        vals.append(x); bases.append(b)
    lens = [len(v) for v in vals]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    val = cast(np.concatenate(vals), dtype)
    for a in (val, off, mean, sd):
        a.setflags(write=False)
    return dict(val=val, off=off, base=np.concatenate(bases), mean=mean, sd=sd)


@functools.lru_cache(maxsize=None)
def parity_expected(k, center, dtype, weighted, clip_rounds):
    p = parity_inputs(k, center, dtype)
    return rescale(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], weighted=weighted, clip_sigma=3.0, clip_rounds=clip_rounds,
                   min_events=PARITY_MIN_EVENTS)


PARITY_CASES = [(k, c, dt, w, r) for k in (1, 5, 8) for c in sorted({0, k - 1}) for dt in ('int16', 'float32', 'float64')
                for w in (True, False) for r in (0, 2)]
