"""Restatement of nmod_kmer_model's definition (include/nanomod_hip.h, K10) and of kmermodel.kmer_codes, for the tests.

int16 rows: Python integers and `fractions` — the exact rational mean and the exact V = N S2 - S1^2, whose square root is taken to
100 binary digits beyond the point before the one rounding to double.  float rows: math.fsum over the pooled doubles.  kmer_codes:
strings sliced per position.  Nothing here shares code with the package."""
import math
from fractions import Fraction

import numpy as np

NO_CODE, EMPTY, TOO_LARGE, NONFINITE = 64, 4, 8, 16
MAX_DEEP = 2 ** 24 - 1
MAX_KMER_CODES = 65536


def csr(rows, dtype):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    sig = np.concatenate([np.asarray(r, dtype=dtype) for r in rows]) if rows else np.zeros(0, dtype)
    return np.ascontiguousarray(sig.astype(dtype)), off


def as_double(x, dtype):
    """a stored sample as the double the definition takes it as"""
    if np.dtype(dtype) == np.int16:
        return int(x) / 1000.0
    return float(x)


def grid_rows(rng, lengths, level_of, spread=0.2, outliers=0.01, dtype=np.int16):
    """rows on the 3-decimal grid around a level per row, `outliers` of the samples replaced by values over +-5 units; returned in
    `dtype` (int16: milli-units)"""
    rows = []
    for i, n in enumerate(lengths):
        k = np.rint(1000.0 * rng.normal(level_of(i), spread, n))
        out = rng.random(n) < outliers
        k[out] = np.rint(1000.0 * rng.uniform(-5.0, 5.0, int(out.sum())))
        k = np.clip(k, -32767, 32767)
        rows.append(k.astype(np.int16) if np.dtype(dtype) == np.int16 else (k / 1000.0).astype(dtype))
    return rows


def position_status(row, code, ncodes, dtype):
    st = 0
    if code < 0 or code >= ncodes:
        st |= NO_CODE
    if len(row) == 0:
        st |= EMPTY
    if len(row) > MAX_DEEP:
        st |= TOO_LARGE
    if st == 0 and np.dtype(dtype) != np.int16 and not bool(np.all(np.isfinite(np.asarray(row, dtype=np.float64)))):
        st = NONFINITE
    return st


def _sqrt_fraction(v):
    """sqrt of a non-negative integer, as a Fraction good to 2^-100 absolute"""
    return Fraction(math.isqrt(v << 200), 1 << 100)


def kmer_model(rows, codes, ncodes, dtype, keep_lo=None, keep_hi=None):
    """the definition on a list of rows (arrays of `dtype`) and their codes; returns the dict of the device entry"""
    dtype = np.dtype(dtype)
    npos = len(rows)
    status = np.array([position_status(rows[i], int(codes[i]), ncodes, dtype) for i in range(npos)], dtype=np.uint8)
    n_pos = np.zeros(ncodes, np.int64); n_s = np.zeros(ncodes, np.int64); n_c = np.zeros(ncodes, np.int64)
    mean = np.full(ncodes, np.nan); sd = np.full(ncodes, np.nan)
    pooled = {}
    for i in range(npos):
        if status[i]:
            continue
        c = int(codes[i])
        kept = []
        for x in np.asarray(rows[i]).tolist():
            d = as_double(x, dtype)
            if keep_lo is None or (float(keep_lo[c]) <= d and d <= float(keep_hi[c])):
                kept.append(x)
            else:
                n_c[c] += 1
        n_s[c] += len(kept)
        n_pos[c] += 1 if kept else 0
        pooled.setdefault(c, []).extend(kept)
    for c, xs in pooled.items():
        n = len(xs)
        if n == 0:
            continue
        if dtype == np.int16:
            s1 = sum(int(x) for x in xs); s2 = sum(int(x) * int(x) for x in xs)
            mean[c] = float(Fraction(s1, n) / 1000)
            sd[c] = float(_sqrt_fraction(n * s2 - s1 * s1) / n / 1000)
        else:
            d = [float(x) for x in xs]
            m = math.fsum(d) / n
            mean[c] = m
            sd[c] = math.sqrt(math.fsum((x - m) * (x - m) for x in d) / n)
    return dict(n_positions=n_pos, n_samples=n_s, n_clipped=n_c, mean=mean, sd=sd, pos_status=status)


def kmer_string(code, k):
    return ''.join('ACGT'[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def kmer_codes(chrom, strand, pos, base, k, center):
    """the code of every row by slicing strings: the letters at read-direction offsets -center .. k - 1 - center (pos + d on '+',
    pos - d on '-'), all present for that (chrom, strand) — consecutive present positions are one run"""
    table = {}
    for c, s, p, b in zip(chrom, strand, pos, base):
        table[(str(c), str(s), int(p))] = str(b)
    out = []
    for c, s, p in zip(chrom, strand, pos):
        step = -1 if str(s) == '-' else 1
        letters = [table.get((str(c), str(s), int(p) + step * d)) for d in range(-center, k - center)]
        if any(x is None or x not in 'ACGT' or len(x) != 1 for x in letters):
            out.append(-1)
        else:
            word = ''.join(letters)
            out.append(int(sum('ACGT'.index(ch) * 4 ** (k - 1 - i) for i, ch in enumerate(word))))
    return np.array(out, dtype=np.int32)
