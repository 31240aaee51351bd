"""The definition of nmod_pair_index / nmod_site_pairs (K16, include/nanomod_hip.h) restated for the tests: the pair index by brute
force, the counts by a plain loop over reads and covered site pairs, p_fisher in exact rational arithmetic, and the double recurrence
of the header step for step (both orders: one thread, one wave).

The gate between the recurrence and the exact value
---------------------------------------------------
u = 2^-53; every count below is of correctly rounded operations, each a factor (1 + e), |e| <= u, on a non-negative value, so a value
that went through m of them is exact up to (1 + u)^m, m u to first order.  L is the size of the support, n_up = hi - mode and
n_dn = mode - lo the weights above and below the mode: n_up + n_dn = L - 1.
The weights.  Relative to the mode the exact weight of table x is a product of d = |x - mode| exact rational ratios.  The recurrence
forms each ratio by one rounded division of two integers that are exact as doubles (products below 2^52 while N < 2^26), and the
weight by multiplying the d rounded ratios: d - 1 multiplications in any order of association (the one thread's left to right, the
wave's lane scan joined to the carry of the tiles before), since the multiplication by w(mode) = 1.0, or by the first carry 1.0, is
exact.  At most 2 d - 1 operations per weight.  No operation overflows: every partial product on one side of the mode is a product of
ratios <= 1.  (One that underflows is an absolute error, not a relative one: the floor below.)
The sums, one thread.  U adds the weights above the mode in ascending distance from 0.0: the weight at distance d goes through the
n_up - d additions after its own (its own is exact for d = 1 and counted with the one before otherwise) and through the two of
(1.0 + U) + D: at most n_up - d + 2, with 2 d - 1 for the weight itself n_up + d + 1 <= 2 n_up + 1 <= 2 L - 1.  The same below the
mode.  In T a skipped weight adds 0.0, which is exact.  So S and T are each exact up to (1 + u)^(2 L - 1), and with the division
    |p / p_exact - 1| <= (4 L - 1) u + O(u^2)  <=  (4 L + 8) u,
the gate the issue states; the slack of 9 u covers the second-order terms for every L below 2^24.
The sums, one wave.  A lane adds its weights in tile order, ceil(n_up / 64) + ceil(n_dn / 64) <= (L - 1) / 64 + 2 terms, then the
wave sum adds 4 exchange steps and 3 rows (the first row is added to 0.0), then 1.0: per weight at most (L - 1) / 64 + 1 + 8
additions on top of its 2 d - 1 <= 2 L - 3.  S and T are exact up to (1 + u)^(2 L + L / 64 + 6) and
    |p / p_exact - 1| <= (4 L + L / 32 + 13) u + O(u^2)  <=  (4 L + L / 32 + 16) u:
the wave's order needs the further term L / 32 + 8 and gate() adds it for the supports the wave computes.
(What occurs is far smaller: 300 random tables with margins up to 2 000 gave at most 0.67 L u in either order.)
Floor: where p_exact < 1e-290 the weights of the tail come within 2^60 of the subnormal range, where a rounding is absolute; the only
requirement is then DBL_MIN <= p <= 1e-289.

The tie rule.  A table x belongs to the tail iff w(x) <= w(n11) (1 + 1e-7).  A rounding decides that only if the exact ratio
w(x) / w(n11) lies within the rounding error of 1 + 1e-7; near_tie() reports a table with a ratio within 1e-9 of it, far more than
any rounding error here (<= 4 L u < 1e-12), and the tests assert that none of their tables is one.  Exactly equal weights (ratio 1)
are on the tail side by 1e-7 and are never near.
"""
import math
from fractions import Fraction

import numpy as np

POS_MASK = (1 << 40) - 1
DBL_MIN = 2.2250738585072014e-308
U = 2.0 ** -53
SLACK = 1.0 + 1e-7                                   # the double the device multiplies by
THREAD_MAX = 64                                      # NMOD_PAIRS_THREAD_MAX; test_site_pairs.py checks it against the header
TOO_FEW, DEGENERATE = 1, 2


def gate(L, thread_max=THREAD_MAX):
    """the relative error allowed between the recurrence and the exact p over a support of L tables (p_exact >= 1e-290): derived above"""
    return (4 * L + 8 + (L / 32.0 + 8 if L > thread_max else 0)) * U


def call(score, thr):
    """1: MOD, 0: CAN, 2: none (NaN is none)"""
    return 1 if score >= thr else (0 if score <= -thr else 2)


def pair_index_ref(key, max_dist):
    """poff (int64[nsites + 1]) by brute force"""
    key = [int(k) for k in key]
    cnt = []
    for a, ka in enumerate(key):
        c = 0
        for kb in key[a + 1:]:
            if kb >> 40 != ka >> 40 or (kb & POS_MASK) - (ka & POS_MASK) > max_dist:
                break
            c += 1
        cnt.append(c)
    return np.concatenate(([0], np.cumsum(np.array(cnt, dtype=np.int64)))).astype(np.int64)


def counts_ref(cs, start, roff, score, key, poff, thr):
    """counts (int32[4 npairs]) by a loop over the reads and the pairs of sites each covers with a call"""
    key = np.asarray(key, dtype=np.int64)
    counts = np.zeros(4 * int(poff[-1]), dtype=np.int32)
    for r in range(len(cs)):
        b, n = int(roff[r]), int(roff[r + 1] - roff[r])
        if n <= 0:
            continue
        lo = np.searchsorted(key, (int(cs[r]) << 40) | int(start[r]), 'left')
        hi = np.searchsorted(key, (int(cs[r]) << 40) | (int(start[r]) + n - 1), 'right')
        called = []
        for s in range(lo, hi):
            pos = int(key[s]) & POS_MASK
            i = int(start[r]) + n - 1 - pos if cs[r] & 1 else pos - int(start[r])
            c = call(score[b + i], thr)
            if c != 2:
                called.append((s, c))
        for x, (sa, ca) in enumerate(called):
            reach = sa + 1 + int(poff[sa + 1] - poff[sa])
            for sb, cb in called[x + 1:]:
                if sb >= reach:
                    break
                counts[4 * (int(poff[sa]) + (sb - sa - 1)) + 2 * ca + cb] += 1
    return counts


def margins(n11, n10, n01, n00):
    N = n11 + n10 + n01 + n00
    r1, c1 = n11 + n10, n11 + n01
    lo, hi = max(0, r1 + c1 - N), min(r1, c1)
    mode = min(max(((r1 + 1) * (c1 + 1)) // (N + 2), lo), hi)
    return N, r1, c1, lo, hi, mode


def exact_weights(n11, n10, n01, n00):
    """the hypergeometric weights of the support as integers (comb(r1, x) comb(r0, c1 - x)), and lo"""
    N, r1, c1, lo, hi, _ = margins(n11, n10, n01, n00)
    return [math.comb(r1, x) * math.comb(N - r1, c1 - x) for x in range(lo, hi + 1)], lo


def fisher_exact(n11, n10, n01, n00):
    """p_fisher in exact rational arithmetic (a Fraction), the tie slack as the Fraction of the double 1 + 1e-7"""
    w, lo = exact_weights(n11, n10, n01, n00)
    cut = Fraction(w[n11 - lo]) * Fraction(SLACK)
    return min(Fraction(sum(v for v in w if v <= cut), sum(w)), Fraction(1))


def near_tie(n11, n10, n01, n00, slack=SLACK, width=1e-9):
    """whether some table of the support has w(x) / w(n11) within `width` of the slack: rounding could then decide the tie rule"""
    w, lo = exact_weights(n11, n10, n01, n00)
    wo = w[n11 - lo]
    lo_r, hi_r = Fraction(slack) - Fraction(width), Fraction(slack) + Fraction(width)
    return any(lo_r * wo <= v <= hi_r * wo for v in w)


def _up(x, N, r1, c1):
    return np.float64((c1 - x) * (r1 - x)) / np.float64((x + 1) * (N - c1 - r1 + x + 1))


def _down(x, N, r1, c1):
    return np.float64(x * (N - c1 - r1 + x)) / np.float64((c1 - x + 1) * (r1 - x + 1))


def _finish(T, S):
    with np.errstate(all='ignore'):
        p = T / S
    return float(max(min(p, np.float64(1.0)), np.float64(DBL_MIN)))


def fisher_thread(n11, n10, n01, n00):
    """the header's recurrence in the order of one thread"""
    N, r1, c1, lo, hi, mode = margins(n11, n10, n01, n00)
    one, zero = np.float64(1.0), np.float64(0.0)
    with np.errstate(all='ignore'):
        wo = one
        if n11 > mode:
            for x in range(mode, n11):
                wo = wo * _up(x, N, r1, c1)
        else:
            for x in range(mode, n11, -1):
                wo = wo * _down(x, N, r1, c1)
        cut = wo * np.float64(SLACK)
        Usum = TU = D = TD = zero
        w = one
        for x in range(mode, hi):
            w = w * _up(x, N, r1, c1)
            Usum = Usum + w
            TU = TU + (w if w <= cut else zero)
        w = one
        for x in range(mode, lo, -1):
            w = w * _down(x, N, r1, c1)
            D = D + w
            TD = TD + (w if w <= cut else zero)
        S = (one + Usum) + D
        T = ((one if one <= cut else zero) + TU) + TD
    return _finish(T, S)


def _wave_sum(v):
    """the library's wave sum of 64 doubles (wave_ops.hpp: wave_sum_f64)"""
    l = np.arange(64)
    v = v + v[l ^ 1]
    v = v + v[l ^ 2]
    v = v + v[(l & ~7) | (7 - (l & 7))]
    v = v + v[(l & ~15) | (15 - (l & 15))]
    r = np.float64(0.0)
    for row in range(4):
        r = r + v[16 * row]
    return r


def _wave_side(up, N, r1, c1, lo, hi, mode):
    """the weights of one side of the mode as the wave computes them: a list of (64 distances - 1, 64 weights) per tile"""
    length = hi - mode if up else mode - lo
    lanes = np.arange(64)
    carry = np.float64(1.0)
    tiles = []
    for t0 in range(0, length, 64):
        k = t0 + lanes
        r = np.zeros(64)
        for i in range(64):
            if k[i] < length:
                x = mode + int(k[i]) if up else mode - int(k[i])
                r[i] = _up(x, N, r1, c1) if up else _down(x, N, r1, c1)
        v = r.copy()
        d = 1
        while d < 64:
            o = v.copy()
            v[d:] = o[d:] * o[:-d]
            d *= 2
        w = carry * v
        tiles.append((k, w))
        carry = w[63]
    return tiles


def fisher_wave(n11, n10, n01, n00):
    """the header's recurrence in the order of one wave"""
    N, r1, c1, lo, hi, mode = margins(n11, n10, n01, n00)
    with np.errstate(all='ignore'):
        sides = [_wave_side(True, N, r1, c1, lo, hi, mode), _wave_side(False, N, r1, c1, lo, hi, mode)]
        wo = np.float64(1.0)
        if n11 != mode:
            ko = abs(n11 - mode) - 1
            for k, w in sides[0 if n11 > mode else 1]:
                if k[0] <= ko <= k[63]:
                    wo = w[ko - k[0]]
        cut = wo * np.float64(SLACK)
        s, tl = np.zeros(64), np.zeros(64)
        for side in sides:
            for _, w in side:
                s = s + w
                tl = tl + np.where(w <= cut, w, 0.0)
        S = np.float64(1.0) + _wave_sum(s)
        T = (np.float64(1.0) if np.float64(1.0) <= cut else np.float64(0.0)) + _wave_sum(tl)
    return _finish(T, S)


def fisher_recurrence(n11, n10, n01, n00, thread_max=THREAD_MAX):
    """p_fisher as the device computes it: the order follows the pair's own support"""
    _, _, _, lo, hi, _ = margins(n11, n10, n01, n00)
    return fisher_thread(n11, n10, n01, n00) if hi - lo + 1 <= thread_max else fisher_wave(n11, n10, n01, n00)


def pair_stats_ref(counts, min_reads, poff=None):
    """log_or, se, phi, p_fisher (by the recurrence), status — and first, second with poff — of int32[4 npairs] counts"""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    m = len(c)
    res = dict(log_or=np.full(m, np.nan), se=np.full(m, np.nan), phi=np.full(m, np.nan), p_fisher=np.full(m, np.nan),
               status=np.zeros(m, dtype=np.uint8))
    for j in range(m):
        n00, n01, n10, n11 = (int(v) for v in c[j])
        N, r1, c1, _, _, _ = margins(n11, n10, n01, n00)
        r0, c0 = N - r1, N - c1
        few, deg = N < min_reads, 0 in (r1, r0, c1, c0)
        res['status'][j] = (TOO_FEW if few else 0) | (DEGENERATE if deg else 0)
        if few:
            continue
        h11, h10, h01, h00 = (np.float64(v) + 0.5 for v in (n11, n10, n01, n00))
        res['log_or'][j] = np.log((h11 * h00) / (h10 * h01))
        res['se'][j] = np.sqrt(((1.0 / h11 + 1.0 / h10) + 1.0 / h01) + 1.0 / h00)
        if not deg:
            res['phi'][j] = np.float64(n11 * n00 - n10 * n01) / np.sqrt(np.float64(r1 * r0) * np.float64(c1 * c0))
        res['p_fisher'][j] = fisher_recurrence(n11, n10, n01, n00)
    if poff is not None:
        poff = np.asarray(poff, dtype=np.int64)
        first = np.repeat(np.arange(len(poff) - 1), np.diff(poff))
        res['first'] = first.astype(np.int32)
        res['second'] = (first + 1 + (np.arange(m) - poff[first])).astype(np.int32)
    return res


# what a device value may differ by from pair_stats_ref: log of a ratio with one rounding (absolute u on the log, and the log's own
# last bit); se and phi: a handful of correctly rounded operations
def close_log_or(got, want):
    return np.all((np.abs(got - want) <= 8 * U * (1.0 + np.abs(want))) | (np.isnan(got) & np.isnan(want)))


def close_rel(got, want, ulps=8):
    return np.all((np.abs(got - want) <= ulps * U * np.abs(want)) | (np.isnan(got) & np.isnan(want)))


def p_within_gate(got, table):
    """a device p_fisher against the exact value of its table (n11, n10, n01, n00): the gate above, or the floor rule"""
    n11, n10, n01, n00 = table
    _, _, _, lo, hi, _ = margins(n11, n10, n01, n00)
    exact = fisher_exact(n11, n10, n01, n00)
    if exact < Fraction(1e-290):
        return DBL_MIN <= got <= 1e-289
    return abs(Fraction(got) / exact - 1) <= Fraction(gate(hi - lo + 1))


def cooccur_inputs(seed=165, n_reads=160, genome_len=400):
    """A read-level sample for the chain K13 -> K16, in readllr_ref.chain_inputs' manner: reads of 150 .. 250 events from a 3-mer model
    (center 0) over one short reference, both strands, every read covering three planted bases A < B < C twenty apart.  The modified
    table lies 3 spreads higher at the k-mers that cover a planted base.  A and B are modified on the same half of the reads (by the
    read's number), C on a half drawn independently (seed 165: of seeds 161 .. 174 the one whose draw of C splits the
    reads most evenly against A on both strands; 161 drew a C that leans against A at p = 0.007).  (reads, model, alt_model, (A, B, C), modified: bool[n_reads, 3])"""
    import readllr_ref as RF
    import rescale_ref as R
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    planted = (genome_len // 2 - 20, genome_len // 2, genome_len // 2 + 20)
    lo, hi = RF.kmer_window(k, center)
    mean1 = mean.copy()
    plan = []
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(150, 251))
        s0 = int(rng.integers(max(0, planted[2] - n + 20), min(genome_len - n, planted[0] - 20) + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        covers = []
        for p in planted:
            j = int(np.flatnonzero(pos == p)[0])
            cover = np.arange(j - lo, j + hi + 1)                            # the events whose k-mer holds the planted base
            mean1[codes[cover]] = mean[codes[cover]] + 3.0 * sd[codes[cover]]
            covers.append(cover)
        plan.append((minus, s0, b, codes, covers, rng.normal(size=n), bool(rng.integers(0, 2))))
    chrom, strand, start, vals, bases = [], [], [], [], []
    modified = np.zeros((n_reads, 3), bool)
    for r, (minus, s0, b, codes, covers, noise, mod_c) in enumerate(plan):
        modified[r] = ((r // 2) % 2 == 0, (r // 2) % 2 == 0, mod_c)
        level = mean[codes].copy()
        for cover, m in zip(covers, modified[r]):
            if m:
                level[cover] = mean1[codes[cover]]
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint((level + sd[codes] * noise) * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    ones = np.ones(4 ** k, np.int64)
    return (reads, dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones),
            dict(k=k, center=center, mean=mean1, sd=sd.copy(), n_positions=ones), planted, modified)
