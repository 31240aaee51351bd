"""nmod_read_llr / nmod_site_llr (K13) restated in numpy from the text of include/nanomod_hip.h, the mpmath values the restatement is
pinned against, the gates of the GPU tests, and the seeded inputs the CPU and GPU tests share.  Nothing here calls the library.  The
event codes are rescale_ref's (K11's definition, word for word); the pivot is readcalls_ref's.

The gates are derived, not tuned.  Of the definition only g (the device's log) and exp can differ from numpy: every other operation
is a correctly rounded IEEE operation in a fixed order.  With g within 8 ulp, a window sum of up to 129 terms differs by at most
8 * 2^-53 * sum |g_i| from the g and by nothing else (the same terms are added in the same order); GATE_L = 2^-44 * sum (|g_i| + |d_i|)
is about twice the worst case of an 8-ulp g plus 128 roundings of partial sums, were the order not fixed."""
import functools

import numpy as np

import readcalls_ref as Q
import rescale_ref as R

TOO_LARGE = Q.TOO_LARGE
MAX_DEEP = Q.MAX_DEEP
WAVE_MAX = Q.WAVE_MAX
MAX_NB = Q.MAX_NB
DBL_MIN = Q.DBL_MIN
LLR_MAX = 1e300
PRIOR_LOGIT_MAX = 700.0
pivot = Q.pivot

GATE_L_UNIT = 2.0 ** -44                          # gate_L(j) = GATE_L_UNIT * sum over the window of |g_i| + |d_i|
GATE_LLR_UNIT = 2.0 ** -49                        # llr_j within GATE_LLR_UNIT * max(|g|, |d|, |llr|)
GATE_P_EXTRA = 2.0 ** -49                         # p_mod within gate_L(j) + GATE_P_EXTRA, relative

PIN_Z0 = (0.0, 1e-3, 1.0, 8.0, 40.0, 1e3)
PIN_GAP = (0.0, 0.5, 3.0)                         # mu1 - mu0 in spreads of the unmodified model
PIN_RATIO = (1.0, 0.5, 2.0)                       # sd1 / sd0
PIN_T = (-800.0, -745.0, -40.0, -1e-3, 0.0, 1e-3, 40.0, 800.0)
PIN_GATE = 1e-13


def kmer_window(k, center):
    """the events whose k-mer holds the base of event j: (nb_lo, nb_hi)"""
    return k - 1 - center, center


def code_table(mean0, sd0, mean1, sd1):
    """per code: usable, and g = log(sd0 / sd1) (0 where unusable)"""
    m0, s0, m1, s1 = (np.asarray(a, np.float64) for a in (mean0, sd0, mean1, sd1))
    with np.errstate(invalid='ignore'):
        usable = np.isfinite(m0) & np.isfinite(s0) & np.isfinite(m1) & np.isfinite(s1) & (s0 > 0.0) & (s1 > 0.0)
    g = np.zeros(len(m0))
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        g[usable] = np.log(s0[usable] / s1[usable])
    return usable, g


def posterior(t):
    """p_mod of t = L + prior_logit: t >= 0 ? 1 / (1 + exp(-t)) : exp(t) / (1 + exp(t))"""
    t = np.asarray(t, np.float64)
    p = np.full(t.shape, np.nan)
    up = t >= 0.0
    p[up] = 1.0 / (1.0 + np.exp(-t[up]))
    dn = t < 0.0
    q = np.exp(t[dn])
    p[dn] = q / (1.0 + q)
    return p


def score_read(x, codes, mean0, sd0, mean1, sd1, nb_lo, nb_hi, prior_logit=0.0):
    """one read: dict(llr, llr_win, p_mod (NaN where ineligible), elig, gate_llr, gate_L)"""
    n = len(x)
    usable, g_tab = code_table(mean0, sd0, mean1, sd1)
    c = np.where(codes >= 0, codes, 0)
    with np.errstate(invalid='ignore'):
        cand = (codes >= 0) & usable[c] & np.isfinite(x)
    m0, s0, m1, s1 = (np.asarray(a, np.float64)[c] for a in (mean0, sd0, mean1, sd1))
    g, d, llr = np.zeros(n), np.zeros(n), np.full(n, np.nan)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        z0 = (x[cand] - m0[cand]) / s0[cand]
        z1 = (x[cand] - m1[cand]) / s1[cand]
        d[cand] = 0.5 * ((z0 - z1) * (z0 + z1))
        g[cand] = g_tab[c[cand]]
        llr[cand] = g[cand] + d[cand]
        elig = cand & (np.abs(llr) <= LLR_MAX)                   # (NaN: not)
    llr[~elig] = np.nan
    mag = np.where(elig, np.abs(g) + np.abs(d), 0.0)
    with np.errstate(invalid='ignore'):
        gate_llr = GATE_LLR_UNIT * np.where(elig, np.maximum(np.maximum(np.abs(g), np.abs(d)), np.abs(llr)), 0.0)
    if nb_lo == 0 and nb_hi == 0:
        S, G = np.where(elig, llr, 0.0), mag.copy()              # L is llr, the same bits
    else:
        S, G = np.zeros(n), np.zeros(n)
        for sh in range(-nb_lo, nb_hi + 1):                      # the terms in ascending i = j + sh; an event that takes no part adds an exact 0
            lo, hi = max(0, -sh), min(n, n - sh)
            if lo >= hi:
                continue
            part = elig[lo + sh:hi + sh]
            S[lo:hi] = S[lo:hi] + np.where(part, llr[lo + sh:hi + sh], 0.0)
            G[lo:hi] = G[lo:hi] + np.where(part, mag[lo + sh:hi + sh], 0.0)
    L = np.where(elig, S, np.nan)
    p = np.full(n, np.nan)
    p[elig] = posterior(L[elig] + prior_logit)
    return dict(llr=llr, llr_win=L, p_mod=p, elig=elig, gate_llr=gate_llr, gate_L=GATE_L_UNIT * np.where(elig, G, 0.0))


def restate(val, off, base, k, center, mean0, sd0, mean1, sd1, window='kmer', thr=2.5, prior_logit=0.0):
    """the whole entry on host arrays: dict(llr, llr_win, p_mod, gate_llr, gate_L, n_sites, n_mod, n_can, status) and thr_margin =
    min_j(||L_j| - thr| - gate_L(j)): positive means that no device sum within its gate can fall on the other side of a threshold"""
    nb_lo, nb_hi = kmer_window(k, center) if isinstance(window, str) else window
    val, off = np.asarray(val), np.asarray(off, np.int64)
    nreads = len(off) - 1
    bb = R.as_bytes(base)
    nan = lambda: np.full(len(val), np.nan)
    out = dict(llr=nan(), llr_win=nan(), p_mod=nan(), gate_llr=np.zeros(len(val)), gate_L=np.zeros(len(val)),
               n_sites=np.zeros(nreads, np.int32), n_mod=np.zeros(nreads, np.int32), n_can=np.zeros(nreads, np.int32),
               status=np.zeros(nreads, np.uint8), thr_margin=np.inf)
    for i in range(nreads):
        b0, e0 = int(off[i]), int(off[i + 1])
        if e0 - b0 > MAX_DEEP:
            out['status'][i] = TOO_LARGE
            continue
        r = score_read(R.to_double(val[b0:e0]), R.read_codes(bb[b0:e0], k, center), mean0, sd0, mean1, sd1, nb_lo, nb_hi, prior_logit)
        for f in ('llr', 'llr_win', 'p_mod', 'gate_llr', 'gate_L'):
            out[f][b0:e0] = r[f]
        ok, L = r['elig'], r['llr_win']
        out['n_sites'][i] = int(ok.sum())
        out['n_mod'][i] = int((L[ok] >= thr).sum())
        out['n_can'][i] = int((L[ok] <= -thr).sum())
        if ok.any():
            out['thr_margin'] = min(out['thr_margin'], float((np.abs(np.abs(L[ok]) - thr) - r['gate_L'][ok]).min()))
    return out


def site_llr(score, off, thr=2.5):
    score, off = np.asarray(score, np.float64), np.asarray(off, np.int64)
    npos = len(off) - 1
    n_valid, n_mod, n_can, frac = np.zeros(npos, np.int32), np.zeros(npos, np.int32), np.zeros(npos, np.int32), np.full(npos, np.nan)
    for i in range(npos):
        s = score[off[i]:off[i + 1]]
        with np.errstate(invalid='ignore'):
            n_valid[i], n_mod[i], n_can[i] = int(np.isfinite(s).sum()), int((s >= thr).sum()), int((s <= -thr).sum())
        if n_mod[i] + n_can[i]:
            frac[i] = np.float64(n_mod[i]) / np.float64(n_mod[i] + n_can[i])
    return dict(n_valid=n_valid, n_mod=n_mod, n_can=n_can, frac=frac)


# --------------------------------------------------------------------------------------------------------------------- mpmath pins

def pin_llr_cases():
    """(x, mu0, sd0, mu1, sd1) of the pins, as doubles: |z0| of PIN_Z0 (both signs) crossed with the level gaps and the spread ratios,
    over mu0 = 0 and sd0 = 1 (x is z0 itself) and over mu0 = 0.25, sd0 = 0.5"""
    out = []
    for mu0, sd0 in ((0.0, 1.0), (0.25, 0.5)):
        for z in PIN_Z0:
            for s in ((z, -z) if z else (z,)):
                for gap in PIN_GAP:
                    for ratio in PIN_RATIO:
                        out.append((mu0 + s * sd0, mu0, sd0, mu0 + gap * sd0, ratio * sd0))
    return out


def mp_llr(x, mu0, sd0, mu1, sd1):
    """ln N(x; mu1, sd1^2) - ln N(x; mu0, sd0^2) of the doubles as they are, in 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    x, mu0, sd0, mu1, sd1 = (mp.mpf(float(v)) for v in (x, mu0, sd0, mu1, sd1))
    return mp.log(sd0 / sd1) + (((x - mu0) / sd0) ** 2 - ((x - mu1) / sd1) ** 2) / 2


def mp_posterior(t):
    import mpmath as mp
    mp.mp.dps = 50
    return 1 / (1 + mp.exp(-mp.mpf(float(t))))


def pin_agreement():
    """worst relative deviation of the restatement from mpmath over the pins: (llr, p_mod); raises where the restatement is not exactly 0
    (llr) or exactly 0 / 1 (p_mod) where mpmath's value is, or rounds there"""
    worst_l = worst_p = 0.0
    for x, mu0, sd0, mu1, sd1 in pin_llr_cases():
        r = score_read(np.array([x]), np.zeros(1, np.int64), [mu0], [sd0], [mu1], [sd1], 0, 0)
        want = mp_llr(x, mu0, sd0, mu1, sd1)
        got = float(r['llr'][0])
        assert r['elig'][0] and r['llr_win'].tobytes() == r['llr'].tobytes()
        if want == 0:
            assert got == 0.0, (x, mu0, sd0, mu1, sd1, got)
        else:
            worst_l = max(worst_l, abs(float(got / want - 1)))
    for t in PIN_T:
        want = mp_posterior(t)
        got = float(posterior(np.array([t]))[0])
        if float(want) in (0.0, 1.0):
            assert got == float(want), (t, got)
        elif float(want) < DBL_MIN:
            assert abs(got - float(want)) <= 5e-324, (t, got)       # a subnormal: within its last place
        else:
            worst_p = max(worst_p, abs(float(got / want - 1)))
    return worst_l, worst_p


# ------------------------------------------------------------------------------------------------------------------ shared inputs

PARITY_SEED = 41
PARITY_THR = 2.5
PARITY_PRIOR_LOGIT = 0.375
PARITY_KC = ((1, 0), (3, 1), (5, 2), (6, 2))
PARITY_DTYPES = ('int16', 'float32', 'float64')
PARITY_WINDOWS = ((0, 0), 'kmer', (0, 3), (7, 8), (9, 0), (64, 64))


def window_of(window, k, center):
    return kmer_window(k, center) if isinstance(window, str) else window


def parity_lengths(k, lo, hi):
    return [0, 1, k - 1, k, lo + hi, lo + hi + 1, 63, 64, 65, 511, 512, 513, WAVE_MAX, WAVE_MAX + 1, 5000, 70000]


def make_alt_model(k, mean, sd, seed=9, holes=True, equal_sd=False):
    """the modified table of a model: levels moved by -3 .. 3 spreads, spreads scaled by 0.5 .. 2 (or equal); with `holes` (k >= 2) a NaN
    level, a NaN spread and a zero spread at codes that are whole in the unmodified table"""
    rng = np.random.default_rng(2000 * k + seed)
    m = 4 ** k
    mean1 = mean + rng.uniform(-3.0, 3.0, m) * np.where(np.isfinite(sd), np.abs(sd), 0.2)
    sd1 = sd.copy() if equal_sd else sd * rng.uniform(0.5, 2.0, m)
    if holes and k >= 2:
        mean1[5], sd1[10], sd1[15] = np.nan, np.nan, 0.0
    return mean1, sd1


@functools.lru_cache(maxsize=None)
def parity_inputs(k, center, window, dtype, equal_sd=False):
    """the parity read set: dict(val, off, base, mean, sd, alt_mean, alt_sd) — every length at which the code takes another path, model
    holes in either table (k >= 2), reads drawn from one table and the other in turn, contaminated values and an 'N' in some reads"""
    lo, hi = window_of(window, k, center)
    rng = np.random.default_rng(PARITY_SEED + 1000 * k + 100 * center + 7 * lo + hi)
    mean, sd = R.make_model(k)
    mean1, sd1 = make_alt_model(k, mean, sd, equal_sd=equal_sd)
    vals, bases = [], []
    for i, n in enumerate(parity_lengths(k, lo, hi)):
        src = (mean, sd) if i % 2 == 0 else (mean1, sd1)
        b, x = R.draw_read(rng, n, k, center, src[0], src[1], 0.0, 1.0, n_letters=2 if i % 3 == 0 else 0)
        vals.append(x); bases.append(b)
    lens = [len(v) for v in vals]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    val = R.cast(np.concatenate(vals), dtype)
    for a in (val, off, mean, sd, mean1, sd1):
        a.setflags(write=False)
    return dict(val=val, off=off, base=np.concatenate(bases), mean=mean, sd=sd, alt_mean=mean1, alt_sd=sd1)


@functools.lru_cache(maxsize=None)
def parity_expected(k, center, window, dtype, equal_sd=False):
    p = parity_inputs(k, center, window, dtype, equal_sd)
    return restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], p['alt_mean'], p['alt_sd'], window, PARITY_THR, PARITY_PRIOR_LOGIT)


PARITY_CASES = [(k, c, w, dt) for (k, c) in PARITY_KC for w in PARITY_WINDOWS for dt in PARITY_DTYPES]

INELIGIBLE_KC = (3, 1)
INELIGIBLE_WINDOW = (2, 2)
TINY_SD_CODE = 20                                 # its sd0 = 1e-200: |llr| beyond NMOD_LLR_MAX for every value but the level itself


@functools.lru_cache(maxsize=None)
def ineligible_inputs(dtype):
    """K12's list — 'N' and lower-case bytes, model holes, NaN and infinite values, a read shorter than k, a read of ineligible events
    only — and a code usable in one table only, and a code whose sd0 = 1e-200"""
    k, center = INELIGIBLE_KC
    rng = np.random.default_rng(5)
    mean, sd = R.make_model(k)                                               # holes at codes 3, 6, 9, 12
    mean1, sd1 = make_alt_model(k, mean, sd)                                 # and at 5, 10, 15: usable in the unmodified table only
    draw_sd = sd.copy()
    sd = sd.copy()
    sd[TINY_SD_CODE] = 1e-200
    b1, x1 = R.draw_read(rng, 400, k, center, mean, draw_sd, 0.0, 1.0)
    b1[[10, 11, 150, 151, 153, 399]] = [ord(c) for c in 'NacgtN']
    b2 = np.tile(np.frombuffer(b'AATACGGCGTAACCCCTTTGGGACCA', np.uint8), 20)  # runs through the holes of both tables and the tiny spread
    x2 = R.draw_values(rng, b2, k, center, mean, draw_sd, 0.0, 1.0)
    b3, x3 = R.draw_read(rng, 300, k, center, mean, draw_sd, 0.0, 1.0)
    if dtype != 'int16':
        x3[[0, 3, 50, 51, 200, 299]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    b4, x4 = R.draw_read(rng, 2, k, center, mean, draw_sd, 0.0, 1.0)         # shorter than k
    b5, x5 = np.full(100, ord('n'), np.uint8), np.zeros(100)                 # nothing eligible
    b6, x6 = R.draw_read(rng, 70, k, center, mean, draw_sd, 0.0, 1.0)
    reads = [(b1, x1), (b2, x2), (b3, x3), (b4, x4), (b5, x5), (b6, x6)]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r[1]) for r in reads])
    val, base = R.cast(np.concatenate([r[1] for r in reads]), dtype), np.concatenate([r[0] for r in reads])
    codes = np.concatenate([R.read_codes(r[0], k, center) for r in reads])
    return dict(val=val, off=off, base=base, mean=mean, sd=sd, alt_mean=mean1, alt_sd=sd1, codes=codes)


def chain_inputs(seed=77, n_reads=200, genome_len=700, shift_sd=3.0):
    """~200 reads of 300 .. 600 events drawn from a 3-mer model (center 0: the k-mer cover is two events before, none after) over one
    short reference, both strands.  The modified table equals the unmodified one but at the k-mers that cover one planted base on either
    strand, whose levels lie 3 spreads higher; half of the reads of each strand are drawn from the modified table at the events that
    cover the planted base.  (reads, model, alt_model, planted position)"""
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    planted = genome_len // 2
    lo, hi = kmer_window(k, center)
    mean1 = mean.copy()
    plan = []
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(300, 601))
        s0 = int(rng.integers(max(0, planted - n + 20), min(genome_len - n, planted - 20) + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        j = int(np.flatnonzero(pos == planted)[0])
        cover = np.arange(j - lo, j + hi + 1)                                # the events whose k-mer holds the planted base
        mean1[codes[cover]] = mean[codes[cover]] + shift_sd * sd[codes[cover]]
        plan.append((minus, s0, b, codes, cover, rng.normal(size=n)))
    chrom, strand, start, vals, bases = [], [], [], [], []
    for r, (minus, s0, b, codes, cover, noise) in enumerate(plan):
        level = mean[codes].copy()
        if (r // 2) % 2 == 0:
            level[cover] = mean1[codes[cover]]
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint((level + sd[codes] * noise) * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    ones = np.ones(4 ** k, np.int64)
    return reads, dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones), dict(k=k, center=center, mean=mean1, sd=sd.copy(), n_positions=ones), planted


def restate_chain(reads, model, alt, window='kmer', thr=2.5, prior_logit=0.0):
    """the restatement chained through the numpy pivot: (per-read restatement, rows, per-position counts)"""
    exp = restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                  window, thr, prior_logit)
    rows = pivot(reads, exp['llr_win'])
    return exp, rows, site_llr(rows['val'], rows['off'], thr)
