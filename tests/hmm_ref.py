"""The definition of nmod_read_sites_count / nmod_read_hmm (include/nanomod_hip.h, K19) restated from the header's text: the entries of
a read, the sequential float64 forward-backward, the same in the device's documented order of products (tiles, chunks, the lane scan,
the carried vector, power-of-two scaling), a 60-digit mpmath version, the states, runs and site counts, and the gates.  Nothing here
calls the library.

THE GATES are derived, not tuned.  u = 2^-53.  Every quantity of the chain is a sum of products of non-negative terms, so relative
errors add and nothing cancels.  To first order:
  a step matrix entry (T_j diag(e_j)) carries
      ARG_U    the rounding of r = d / length moves rho = exp(-r) by the factor exp(+-r u); rho only enters q + pi rho, whose relative
               change is r u pi rho / (q + pi rho) = r u / (1 + (q / pi) e^r) <= ln(pi / q) u <= ln(1e9) u < 21 u for the allowed pi;
               eps = -expm1(-r) moves by r u e^-r / (1 - e^-r) <= u.                                                     22
      EXP_U    exp, expm1 and log of the device's double-precision library are within 1 ulp = 2 u (HIP's documented bounds;
               glibc's, which this file uses, are below that): rho or eps                                                 2
      the product pi rho (or pi eps, q eps) and the sum with q (or pi)                                                    2
      the emission exp(-|s|), 2 u, and the product with it                                                                3
  = STEP_U = 29;  a 2 x 2 product or a vector step adds 2 u per entry (a product and a sum of products).
  The vector at step k has passed k + 1 step matrices and, per tile, the vector steps of its thread's path ((W - 1) wave totals, the
  lane before, CHUNK replayed steps), each matrix on that path being CHUNK - 1 chunk products and six scan products deep:
      PATH_U(W) = 2 ((W - 1) + 1 + CHUNK) + 2 W (CHUNK - 1 + 6)       per tile of 64 W CHUNK steps.
  post = a1 b1 / (a0 b0 + a1 b1): the two products, the sum and the division add 4 u, and the relative error of a ratio p1 / (p0 + p1)
  is at most twice that of its terms.  Forward and backward together pass m + 1 step matrices.  So
      G(m) = min(CAP, u (2 (STEP_U (m + 1) + 2 tiles PATH_U) + 4)),   CAP = 1e-12.
  The cap binds from about m = 150: the chain forgets, errors do not in fact accumulate with m, and a looser gate would hide a wrong
  carry.  post is compared as |post - ref| <= G ref + 1e-290 (the floor: an entry that turned subnormal under the scaling).
  ll and ll_indep are compared relative to D = sum_j (|log c_j| + max(s_j, 0)) with the same G, as |ll - ref| <= G (D + 1).  The 1: the
  likelihood itself, a product of the c_j, is known to the relative error G at best, so its logarithm to the absolute error G whatever D
  is; and D is 0 for a read whose scores are all 0 (every e_j is (1, 1), every c_j is q + pi, which is 1 only to within u as doubles),
  where a purely relative gate would ask for an exact 0 of sums that no order of double operations gives."""
import math

import numpy as np

POS_MASK = (1 << 40) - 1
DBL_MAX = 1.7976931348623157e+308
U = 2.0 ** -53
CHUNK = 4                                            # NMOD_HMM_CHUNK; test_read_hmm.py checks both against the header
WAVE_MAX = 1024                                      # NMOD_HMM_WAVE_MAX
NO_SITE = 1
LN2 = 0.6931471805599453
ARG_U, EXP_U = 22, 2
STEP_U = ARG_U + EXP_U + 2 + (EXP_U + 1)
CAP = 1e-12
FLOOR = 1e-290


def threads(m):
    return 64 if m <= WAVE_MAX else 256


def path_u(waves):
    return 2 * ((waves - 1) + 1 + CHUNK) + 2 * waves * (CHUNK - 1 + 6)


def gate(m):
    T = threads(m)
    tiles = -(-m // (T * CHUNK))
    return min(CAP, U * (2 * (STEP_U * (m + 1) + 2 * tiles * path_u(T // 64)) + 4))


# ---------------------------------------------------------------------------------------------------------------- the entries

def entries_ref(cs, start, roff, score, key):
    """hoff (int64[nreads + 1]) and per row site (int32), x (the position, float64) and s (the score)"""
    key = np.asarray(key, np.int64)
    hoff, site, xs, ss = [0], [], [], []
    for r in range(len(cs)):
        n = int(roff[r + 1] - roff[r])
        c, st = int(cs[r]), int(start[r])
        if n > 0 and c >= 0 and 0 <= st <= POS_MASK:
            lo = int(np.searchsorted(key, (c << 40) | st, 'left'))
            hi = int(np.searchsorted(key, (c << 40) | min(st + n - 1, POS_MASK), 'right'))
            for a in range(lo, hi):
                pos = int(key[a]) & POS_MASK
                i = st + n - 1 - pos if c & 1 else pos - st
                v = float(score[roff[r] + i])
                if abs(v) <= DBL_MAX:                # (a NaN compares false)
                    site.append(a); xs.append(float(pos)); ss.append(v)
        hoff.append(len(site))
    return np.array(hoff, np.int64), np.array(site, np.int32), np.array(xs, np.float64), np.array(ss, np.float64)


# ---------------------------------------------------------------------------------------------------------------- the model

def emission(s):
    en = math.exp(-abs(s))
    return (en if s > 0.0 else 1.0), (en if s < 0.0 else 1.0)


def transition(d, pi, q, length):
    r = d / length
    rho, eps = math.exp(-r), -math.expm1(-r)
    return q + pi * rho, pi * eps, q * eps, pi + q * rho


def hmm_seq(x, s, pi, length):
    """The sequential scaled forward-backward of the definition -> dict(post, ll, ll_indep, denom); denom = sum (|log c_j| + max(s_j, 0))"""
    m = len(s)
    q = 1.0 - pi
    if m == 0:
        return dict(post=np.zeros(0), ll=0.0, ll_indep=0.0, denom=0.0)
    al = np.zeros((m, 2))
    ll = ind = denom = 0.0
    a0, a1 = q, pi
    for j in range(m):
        e0, e1 = emission(float(s[j]))
        if j:
            t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), pi, q, length)
            a0, a1 = a0 * t00 + a1 * t10, a0 * t01 + a1 * t11
        a0, a1 = a0 * e0, a1 * e1
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        al[j] = a0, a1
        up = max(float(s[j]), 0.0)
        ll += math.log(c) + up
        ind += math.log(q * e0 + pi * e1) + up
        denom += abs(math.log(c)) + up
    post = np.zeros(m)
    b0 = b1 = 1.0
    for j in range(m - 1, -1, -1):
        p0, p1 = al[j, 0] * b0, al[j, 1] * b1
        post[j] = p1 / (p0 + p1)
        if j:
            e0, e1 = emission(float(s[j]))
            t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), pi, q, length)
            y0, y1 = e0 * b0, e1 * b1
            b0, b1 = t00 * y0 + t01 * y1, t10 * y0 + t11 * y1
            c = b0 + b1
            b0, b1 = b0 / c, b1 / c
    return dict(post=post, ll=ll, ll_indep=ind, denom=denom)


def hmm_mp(x, s, pi, length, dps=60):
    """the same in mpmath at `dps` digits, pi, length, x and s taken as the exact doubles they are; post, ll, ll_indep, denom as mpf"""
    import mpmath as mp
    with mp.workdps(dps):
        m = len(s)
        pi_, L = mp.mpf(float(pi)), mp.mpf(float(length))
        q = mp.mpf(1.0 - float(pi))                  # the double the entry forms on the host
        zero, one = mp.mpf(0), mp.mpf(1)
        E, T = [], [None]
        for j in range(m):
            sj = mp.mpf(float(s[j]))
            E.append((mp.exp(-max(sj, zero)), mp.exp(min(sj, zero))))
            if j:
                r = mp.mpf(float(x[j] - x[j - 1])) / L
                rho, eps = mp.exp(-r), -mp.expm1(-r)
                T.append((q + pi_ * rho, pi_ * eps, q * eps, pi_ + q * rho))
        al, ll, ind, denom = [], zero, zero, zero
        a0, a1 = q, pi_
        for j in range(m):
            if j:
                t00, t01, t10, t11 = T[j]
                a0, a1 = a0 * t00 + a1 * t10, a0 * t01 + a1 * t11
            a0, a1 = a0 * E[j][0], a1 * E[j][1]
            c = a0 + a1
            a0, a1 = a0 / c, a1 / c
            al.append((a0, a1))
            up = max(mp.mpf(float(s[j])), zero)
            ll += mp.log(c) + up
            ind += mp.log(q * E[j][0] + pi_ * E[j][1]) + up
            denom += abs(mp.log(c)) + up
        post = [zero] * m
        b0 = b1 = one
        for j in range(m - 1, -1, -1):
            p0, p1 = al[j][0] * b0, al[j][1] * b1
            post[j] = p1 / (p0 + p1)
            if j:
                t00, t01, t10, t11 = T[j]
                y0, y1 = E[j][0] * b0, E[j][1] * b1
                b0, b1 = t00 * y0 + t01 * y1, t10 * y0 + t11 * y1
                c = b0 + b1
                b0, b1 = b0 / c, b1 / c
        return dict(post=post, ll=ll, ll_indep=ind, denom=denom)


# ---------------------------------------------------------------------------------------------------------------- the device's order

def _exponent(mx):
    return math.frexp(mx)[1] if 0.0 < mx <= DBL_MAX else 0


def _mul(l, r):
    a, b = l[0] * r[0] + l[1] * r[2], l[0] * r[1] + l[1] * r[3]
    c, d = l[2] * r[0] + l[3] * r[2], l[2] * r[1] + l[3] * r[3]
    ex = _exponent(max(a, b, c, d))
    return math.ldexp(a, -ex), math.ldexp(b, -ex), math.ldexp(c, -ex), math.ldexp(d, -ex), l[4] + r[4] + ex


def _vmul(x, m):
    y0, y1 = x[0] * m[0] + x[1] * m[2], x[0] * m[1] + x[1] * m[3]
    ex = _exponent(max(y0, y1))
    return math.ldexp(y0, -ex), math.ldexp(y1, -ex), x[2] + m[4] + ex


_IDENTITY = (1.0, 0.0, 0.0, 1.0, 0)


def _step(bwd, k, m, x, s, pi, q, length):
    if k >= m or (bwd and k == 0):
        return _IDENTITY
    j = m - k if bwd else k
    e0, e1 = emission(float(s[j]))
    t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), pi, q, length) if j > 0 else (1.0, 0.0, 0.0, 1.0)
    return (e0 * t00, e0 * t10, e1 * t01, e1 * t11, 0) if bwd else (t00 * e0, t01 * e1, t10 * e0, t11 * e1, 0)


def _scan(bwd, x, s, pi, q, length):
    """the vectors after steps 0 .. m - 1 and the last carry, in the header's ORDER"""
    m = len(s)
    T = threads(m)
    carry = (1.0, 1.0, 0) if bwd else (q, pi, 0)
    out = [None] * m
    for k0 in range(0, m, T * CHUNK):
        live = min(T, -(-(m - k0) // CHUNK))                    # (the threads beyond hold identities: their products are exact)
        steps = [[_step(bwd, k0 + t * CHUNK + c, m, x, s, pi, q, length) for c in range(CHUNK)] for t in range(T)]
        prod = []
        for t in range(T):
            p = steps[t][0]
            for c in range(1, CHUNK):
                p = _mul(p, steps[t][c])
            prod.append(p)
        for w in range(T // 64):
            lanes = prod[64 * w:64 * w + 64]
            for d in (1, 2, 4, 8, 16, 32):
                lanes = [_mul(lanes[l - d], lanes[l]) if l >= d else lanes[l] for l in range(64)]
            prod[64 * w:64 * w + 64] = lanes
        last = None
        for t in sorted(set(range(live)) | {T - 1}):
            w, l = divmod(t, 64)
            v = carry
            for w2 in range(w):
                v = _vmul(v, prod[64 * w2 + 63])
            if l > 0:
                v = _vmul(v, prod[t - 1])
            for c in range(CHUNK):
                k = k0 + t * CHUNK + c
                if k < m:
                    v = _vmul(v, steps[t][c])
                    out[k] = v
            last = v
        carry = last
    return out, carry


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


def _read_sum(terms, m):
    """a per-entry term summed as the device does: a thread's entries in ascending order, the wave sum, the waves in order"""
    T = threads(m)
    per = np.zeros(T)
    for k in range(m):
        t = (k % (T * CHUNK)) // CHUNK
        per[t] = per[t] + terms[k]
    if T == 64:
        return float(_wave_sum(per))
    tot = np.float64(0.0)
    for w in range(T // 64):
        tot = tot + _wave_sum(per[64 * w:64 * w + 64])
    return float(tot)


def hmm_device_order(x, s, pi, length):
    """The chain in the device's documented order -> dict(post, ll, ll_indep)"""
    m = len(s)
    q = 1.0 - pi
    if m == 0:
        return dict(post=np.zeros(0), ll=0.0, ll_indep=0.0)
    fw, last = _scan(False, x, s, pi, q, length)
    bw, _ = _scan(True, x, s, pi, q, length)
    post = np.zeros(m)
    for j in range(m):
        b = bw[m - 1 - j]
        p0, p1 = fw[j][0] * b[0], fw[j][1] * b[1]
        post[j] = p1 / (p0 + p1)
    ups = [max(float(v), 0.0) for v in s]
    ind = []
    for j in range(m):
        e0, e1 = emission(float(s[j]))
        ind.append(math.log(q * e0 + pi * e1) + ups[j])
    ll = (math.log(last[0] + last[1]) + float(last[2]) * LN2) + _read_sum(ups, m)
    return dict(post=post, ll=ll, ll_indep=_read_sum(ind, m))


# ---------------------------------------------------------------------------------------------------------------- states, runs, counts

def states(post, call_post):
    """1 iff post >= call_post, 0 iff post <= 1 - call_post (the double difference), 2 otherwise"""
    post = np.asarray(post, np.float64)
    lo = 1.0 - call_post
    return np.where(post >= call_post, 1, np.where(post <= lo, 0, 2)).astype(np.uint8)


def band_margin(post, call_post, g):
    """whether each reference posterior is further than its gate (g each) from both thresholds"""
    post = np.asarray(post, np.float64)
    out = np.ones(len(post), bool)
    for thr in (call_post, 1.0 - call_post):
        out &= np.abs(post - thr) > g * post + FLOOR + 2 * U
    return out


def runs(state):
    """the maximal runs of 1 in a state track: (first, last) index arrays, inclusive"""
    one = np.concatenate(([0], (np.asarray(state) == 1).astype(np.int8), [0]))
    d = np.diff(one)
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1


def per_read(hoff, state):
    """n_sites, n_mod, n_can, n_runs (int32 each) of the reads from a state track"""
    n = len(hoff) - 1
    res = {f: np.zeros(n, np.int32) for f in ('n_sites', 'n_mod', 'n_can', 'n_runs')}
    for r in range(n):
        st = state[hoff[r]:hoff[r + 1]]
        res['n_sites'][r] = len(st); res['n_mod'][r] = (st == 1).sum(); res['n_can'][r] = (st == 0).sum(); res['n_runs'][r] = len(runs(st)[0])
    return res


def per_site(site, state, nsites):
    site = np.asarray(site, np.int64)
    return dict(site_n=np.bincount(site, minlength=nsites).astype(np.int32),
                site_mod=np.bincount(site[state == 1], minlength=nsites).astype(np.int32),
                site_can=np.bincount(site[state == 0], minlength=nsites).astype(np.int32))


def read_hmm_ref(cs, start, roff, score, key, pi, length, call_post, chain=hmm_seq):
    """Everything nmod_read_hmm writes, from the restatement `chain` (hmm_seq or hmm_device_order), plus denom (float64[nreads]) and
    gate (float64[nrows], the read's G at every row)"""
    hoff, site, x, s = entries_ref(cs, start, roff, score, key)
    n = len(hoff) - 1
    post = np.zeros(len(site))
    g = np.zeros(len(site))
    ll, ind, denom = np.zeros(n), np.zeros(n), np.zeros(n)
    for r in range(n):
        a, b = int(hoff[r]), int(hoff[r + 1])
        if b > a:
            res = chain(x[a:b], s[a:b], pi, length)
            post[a:b] = res['post']; ll[r] = res['ll']; ind[r] = res['ll_indep']
            denom[r] = res['denom'] if 'denom' in res else hmm_seq(x[a:b], s[a:b], pi, length)['denom']
            g[a:b] = gate(b - a)
    st = states(post, call_post)
    out = dict(hoff=hoff, site=site, x=x, s=s, post=post, state=st, ll=ll, ll_indep=ind, denom=denom, gate=g,
               status=np.where(np.diff(hoff) == 0, NO_SITE, 0).astype(np.uint8))
    out.update(per_read(hoff, st))
    out.update(per_site(site, st, len(key)))
    return out


def post_within(got, ref, g):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) <= g * ref + FLOOR


def ll_within(got, ref, g, denom):
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) <= g * (np.asarray(denom, np.float64) + 1.0)


def planted_run(m, first, last, hi=6.0, lo=-6.0):
    """m scores of `lo` with `hi` at first .. last"""
    s = np.full(m, lo)
    s[first:last + 1] = hi
    return s


# ---------------------------------------------------------------------------------------------------------------- the chain K13 -> K19

CHAIN_THR = 2.5


def chain_inputs(seed=190, n_reads=120, genome_len=640, spacing=12, stretch=8, share=0.4, shift=1.5):
    """A read-level sample for the chain K13 -> K19, in pairs_ref.cooccur_inputs' manner: reads of 200 .. 300 events from a 3-mer model
    (center 0) over one short reference, both strands; the candidate sites are every `spacing`-th base on both strands; the modified
    table lies `shift` spreads higher at every k-mer.  `share` of the reads (by the read's number) carry one stretch of `stretch`
    consecutive candidate sites at which the events whose k-mer holds the site's base have the modified level.
    (reads, model, alt_model, sites: (chrom, strand, pos) arrays, planted: bool[n_reads, n_positions] — the read is modified there)"""
    import readllr_ref as RF
    import rescale_ref as R
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    mean1 = mean + shift * sd
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    site_pos = np.arange(spacing, genome_len - spacing, spacing)
    lo, hi = RF.kmer_window(k, center)
    chrom, strand, start, vals, bases = [], [], [], [], []
    planted = np.zeros((n_reads, len(site_pos)), bool)
    for r in range(n_reads):
        minus = r % 2 == 1
        n = int(rng.integers(200, 301))
        s0 = int(rng.integers(0, genome_len - n + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        level = mean[codes].copy()
        covered = np.flatnonzero((site_pos >= s0 + 4) & (site_pos <= s0 + n - 5))
        if r % 5 < round(5 * share) and len(covered) >= stretch:
            first = int(rng.integers(0, len(covered) - stretch + 1))
            for a in covered[first:first + stretch]:
                j = int(np.flatnonzero(pos == site_pos[a])[0])
                cover = np.arange(j - lo, j + hi + 1)
                level[cover] = mean1[codes[cover]]
                planted[r, a] = True
        chrom.append('chrT'); strand.append('-' if minus else '+'); start.append(s0); bases.append(b)
        vals.append(np.rint((level + sd[codes] * rng.normal(size=n)) * 1000.0) / 1000.0)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in vals])
    reads = dict(chrom=np.array(chrom), strand=np.array(strand), start=np.array(start, np.int64), off=off,
                 norm_mean=R.cast(np.concatenate(vals), 'int16'), base=np.concatenate(bases).view('S1'))
    ones = np.ones(4 ** k, np.int64)
    ns = len(site_pos)
    sites = (np.array(['chrT'] * (2 * ns)), np.array(['+'] * ns + ['-'] * ns), np.concatenate((site_pos, site_pos)))
    return (reads, dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones), dict(k=k, center=center, mean=mean1, sd=sd.copy(), n_positions=ones),
            sites, planted)


def result_of(ref, reads, key, names=('chrT',)):
    """read_hmm_ref's results in the layout readllr.smooth_reads_llr returns and its writers take (reads, entries, sites, domains)"""
    from nanomod_amd import readllr
    key = np.asarray(key, np.int64)
    nm = np.array(names, dtype=str)
    called = (ref['site_mod'] + ref['site_can']).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(called > 0, ref['site_mod'] / called, np.nan)
    sites = dict(chrom=nm[key >> 41], strand=np.where((key >> 40) & 1, '-', '+').astype('U1'), pos=key & POS_MASK, n=ref['site_n'], n_mod=ref['site_mod'],
                 n_can=ref['site_can'], share=share)
    n = len(ref['hoff']) - 1
    table = dict(index=np.arange(n, dtype=np.int64), chrom=np.asarray(reads['chrom']).astype(str), strand=np.asarray(reads['strand']).astype(str),
                 **{f: ref[f] for f in ('n_sites', 'n_mod', 'n_can', 'n_runs', 'll', 'll_indep', 'status')})
    return dict(reads=table, entries={f: ref[f] for f in ('hoff', 'site', 'post', 'state')}, sites=sites,
                domains=readllr.read_domains(ref['hoff'], ref['site'], ref['state'], ref['post'], sites['pos']))
