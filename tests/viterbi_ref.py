"""The definition of nmod_read_viterbi (include/nanomod_hip.h, K20) restated from the header's text: the sequential float64 Viterbi
recursion with the tie rule, a brute force over all 2^m paths, a 60-digit mpmath version with the score of any given path and the
max-marginals, the same in the device's documented order (tiles, chunks, the lane scan, the carried vector, the back-pointers of the
replay, the traceback), the counts, and the gates.  The entries of a read, the transition matrix and the order of the read sums are
K19's and come from hmm_ref.  Nothing here calls the library.

THE GATES are derived, not tuned.  u = 2^-53.  Every value of the chain is a sum of step entries, a maximum is exact, so errors are
absolute and are measured against the read's scale
      D = max(|log q|, |log pi|) + sum_j max_rc |L_j[r][c]| (its finite entries) + sum_j max(s_j, 0),
which bounds the magnitude of every partial sum of every path, of every matrix entry of the scan and of S.  max(|log q|, |log pi|)
>= ln 2, and for j >= 1 max(|log(pi eps)|, |log(q eps)|) >= ln 2, so D >= m ln 2.
  A step entry log(T[r][c]) + le[c] carries
      STEP_ABS   T[r][c] is known to the relative error ARG_U + EXP_U + 2 = 26 u (hmm_ref's derivation: the rounding of d / length,
                 exp or expm1, the product and the sum), which moves its logarithm by 26 u absolutely;                       26
                 the off-diagonal entries are log pi + log eps and log q + log eps: eps is known to 3 u, its logarithm moves by as much,
                 and log pi, log q and the sum are counted below: inside the same bound;
      STEP_REL   a log is within 1 ulp = 2 u of its size (log pi and log eps have one sign, so their errors add to 2 u |log(pi eps)|),
                 their sum rounds once and the addition of le (exact itself) once more, u |L| <= u D each.                     4
  A pass goes through at most m <= D / ln 2 steps, so its absolute part is at most 26 / ln 2 < STEP_U = 38 roundings of size u D, and
  its relative part sum_j 4 u |L_j| <= 4 u D.
  Every (max, +) product or vector step adds ONE rounding of at most u D (a sum; the maximum is exact).  The vector at step k has passed,
  per tile, the vector steps of its thread's path ((W - 1) wave totals, the lane before, CHUNK replayed steps), each matrix on that
  path being CHUNK - 1 chunk products and six scan products deep:
      PATH_V(W) = ((W - 1) + 1 + CHUNK) + W (CHUNK - 1 + 6)        per tile of 64 W CHUNK steps
  (half of K19's PATH_U: one operation a product, not two).  S adds CHUNK tiles entries in a thread, eight steps of the wave sum and the
  W waves: SUM_V = CHUNK tiles + 8 + W.  The last operations (the sum of the vector and S; the two sums and the difference of delta, at
  most 2 D each) are 6.  Forward and backward, or the device's scores of two paths, double everything but S:
      G(m) = min(CAP, u (2 (38 + 4 + tiles PATH_V(W)) + SUM_V + 6)),   CAP = 1e-12, K19's cap (it would bind from about 400 tiles).
  vit and delta are compared as |got - ref| <= G (D + 1); the 1 as in hmm_ref (D is never below ln 2 here, it only keeps K19's form).
  A reference delta of infinite size (no path through one of the states: never, T has no zero) does not occur.
  OPTIMALITY.  The device's path is the chain of its own back-pointers.  A back-pointer is decided between two sums the device knows to
  G (D + 1) / 2 each, so a decision whose exact margin exceeds G (D + 1) is the exact one, and a chain of exact decisions is an optimal
  path.  A decision inside that margin may go either way and costs the path at most its exact margin (nothing at an exact tie).  So
      score(device path) >= optimum - G (D + 1) - (the sum of the exact margins of the NEAR decisions, those within G (D + 1)),
  and the reference counts the near decisions of a read and sums their margins (`near`, `near_loss`: 0 and 0 on every fixture without
  constructed ties; at an exact tie the margin is 0).  The same argument gives the path itself: where the reference's |delta_j| exceeds
  G (D + 1) + near_loss, every path within that of the optimum has the optimal state at j, so path_j is the reference's."""
import functools
import math

import numpy as np

import hmm_ref as H

U = H.U
CHUNK, WAVE_MAX, NO_SITE = H.CHUNK, H.WAVE_MAX, H.NO_SITE
LN2 = 0.6931471805599453
STEP_ABS, STEP_REL = 26, 4
STEP_U = 38                                           # STEP_ABS / ln 2, rounded up
assert STEP_ABS / LN2 < STEP_U
CAP = 1e-12
NINF = -math.inf


def path_v(waves):
    return ((waves - 1) + 1 + CHUNK) + waves * (CHUNK - 1 + 6)


def gate(m):
    T = H.threads(m)
    tiles = -(-m // (T * CHUNK))
    return min(CAP, U * (2 * (STEP_U + STEP_REL + tiles * path_v(T // 64)) + (CHUNK * tiles + 8 + T // 64) + 6))


def vmax(u, v):
    """the header's MAX: v where v > u, u otherwise"""
    return v if v > u else u


# ---------------------------------------------------------------------------------------------------------------- the model

def log_emission(s):
    return (-s if s > 0.0 else 0.0), (s if s < 0.0 else 0.0)


def step(j, x, s, pi, q, length):
    """L_j as (l00, l01, l10, l11), float64, in the header's operations"""
    le0, le1 = log_emission(float(s[j]))
    if j == 0:
        return le0, NINF, NINF, le1
    r = float(x[j] - x[j - 1]) / length
    rho, eps = math.exp(-r), -math.expm1(-r)
    leps = math.log(eps)
    return math.log(q + pi * rho) + le0, (math.log(pi) + leps) + le1, (math.log(q) + leps) + le0, math.log(pi + q * rho) + le1


def scale(x, s, pi, length):
    """D of the docstring"""
    q = 1.0 - pi
    d = max(abs(math.log(q)), abs(math.log(pi)))
    for j in range(len(s)):
        d += max(abs(v) for v in step(j, x, s, pi, q, length) if v != NINF) + max(float(s[j]), 0.0)
    return d


def _traceback(psi, z_last):
    m = len(psi)
    path = np.zeros(m, np.uint8)
    z = z_last
    for j in range(m - 1, -1, -1):
        path[j] = z
        if j:
            z = (psi[j] >> z) & 1
    return path


def viterbi_seq(x, s, pi, length):
    """The sequential float64 recursion of the definition -> dict(path, vit, delta)"""
    m = len(s)
    q = 1.0 - pi
    if m == 0:
        return dict(path=np.zeros(0, np.uint8), vit=0.0, delta=np.zeros(0))
    a = np.zeros((m, 2))
    psi = [0] * m
    a0, a1 = math.log(q), math.log(pi)
    for j in range(m):
        l00, l01, l10, l11 = step(j, x, s, pi, q, length)
        s00, s10, s01, s11 = a0 + l00, a1 + l10, a0 + l01, a1 + l11
        psi[j] = (1 if s10 > s00 else 0) | (2 if s11 > s01 else 0)
        a0, a1 = vmax(s00, s10), vmax(s01, s11)
        a[j] = a0, a1
    b = np.zeros((m, 2))
    b0 = b1 = 0.0
    for j in range(m - 1, 0, -1):
        l00, l01, l10, l11 = step(j, x, s, pi, q, length)
        b0, b1 = vmax(b0 + l00, b1 + l01), vmax(b0 + l10, b1 + l11)
        b[j - 1] = b0, b1
    up = 0.0
    for v in s:
        up += max(float(v), 0.0)
    return dict(path=_traceback(psi, 1 if a[m - 1, 1] > a[m - 1, 0] else 0), vit=vmax(a[m - 1, 0], a[m - 1, 1]) + up,
                delta=(a[:, 1] + b[:, 1]) - (a[:, 0] + b[:, 0]))


def path_score(path, x, s, pi, length):
    """the log-probability of one path on ll's scale, float64 (math.fsum of the definition's terms)"""
    q = 1.0 - pi
    terms = [math.log(pi) if path[0] else math.log(q)]
    for j in range(len(s)):
        l = step(j, x, s, pi, q, length)
        terms.append(l[2 * int(path[j - 1] if j else path[0]) + int(path[j])])
        terms.append(max(float(s[j]), 0.0))
    return math.fsum(terms)


def brute_force(x, s, pi, length):
    """the largest path_score over all 2^m paths and the paths that reach it"""
    m = len(s)
    scores = [path_score([(p >> j) & 1 for j in range(m)], x, s, pi, length) for p in range(1 << m)]
    best = max(scores)
    return best, [[(p >> j) & 1 for j in range(m)] for p in range(1 << m) if scores[p] == best]


# ---------------------------------------------------------------------------------------------------------------- mpmath

@functools.lru_cache(maxsize=1 << 16)
def _mp_log_transition(pi, length, d, dps):
    """log T at distance d, entry by entry, at `dps` digits (kept per (pi, length, d): the fixtures repeat their gaps)"""
    import mpmath as mp
    with mp.workdps(dps):
        pi_, q = mp.mpf(pi), mp.mpf(1.0 - pi)
        r = mp.mpf(d) / mp.mpf(length)
        rho, eps = mp.exp(-r), -mp.expm1(-r)
        return mp.log(q + pi_ * rho), mp.log(pi_ * eps), mp.log(q * eps), mp.log(pi_ + q * rho)


class MpChain:
    """the chain of one read at 60 digits, pi, length, x and s taken as the exact doubles they are: opt (the optimum on ll's scale),
    delta (the max-marginal margins), path (the recursion's, under the tie rule), scale (D), near and near_loss at a given gate"""

    def __init__(self, x, s, pi, length, dps=60):
        import mpmath as mp
        self.mp, self.dps, self.m = mp, dps, len(s)
        with mp.workdps(dps):
            m = self.m
            pi_, L = mp.mpf(float(pi)), mp.mpf(float(length))
            q = mp.mpf(1.0 - float(pi))
            zero, ninf = mp.mpf(0), mp.mpf('-inf')
            self.init = (mp.log(q), mp.log(pi_))
            self.steps, self.up = [], zero
            for j in range(m):
                sj = mp.mpf(float(s[j]))
                le0, le1 = -max(sj, zero), min(sj, zero)
                self.up += max(sj, zero)
                if j == 0:
                    self.steps.append((le0, ninf, ninf, le1))
                else:
                    l00, l01, l10, l11 = _mp_log_transition(float(pi), float(length), float(x[j] - x[j - 1]), dps)
                    self.steps.append((l00 + le0, l01 + le1, l10 + le0, l11 + le1))
            self.scale = float(max(abs(self.init[0]), abs(self.init[1])) + sum((max(abs(v) for v in st if v != ninf) for st in self.steps), zero) + self.up)
            a0, a1 = self.init
            self.a, self.margin, psi = [], [], []
            for j in range(m):
                l00, l01, l10, l11 = self.steps[j]
                s00, s10, s01, s11 = a0 + l00, a1 + l10, a0 + l01, a1 + l11
                psi.append((1 if s10 > s00 else 0) | (2 if s11 > s01 else 0))
                self.margin.append((abs(s10 - s00), abs(s11 - s01)))
                a0, a1 = max(s00, s10), max(s01, s11)
                self.a.append((a0, a1))
            if m:
                self.last_margin = abs(a1 - a0)
                self.opt = max(a0, a1) + self.up
                self.path = _traceback(psi, 1 if a1 > a0 else 0)
                b0 = b1 = zero
                d = [None] * m
                d[m - 1] = float(a1 - a0)
                for j in range(m - 1, 0, -1):
                    l00, l01, l10, l11 = self.steps[j]
                    b0, b1 = max(b0 + l00, b1 + l01), max(b0 + l10, b1 + l11)
                    d[j - 1] = float((self.a[j - 1][1] + b1) - (self.a[j - 1][0] + b0))
                self.delta = np.array(d)
            else:
                self.opt, self.path, self.delta, self.last_margin = zero, np.zeros(0, np.uint8), np.zeros(0), zero

    def path_score_mp(self, path):
        """the log-probability on ll's scale of `path` (0 / 1 per entry), an mpf"""
        mp = self.mp
        with mp.workdps(self.dps):
            if self.m == 0:
                return mp.mpf(0)
            tot = self.init[int(path[0])] + self.up
            for j in range(self.m):
                tot += self.steps[j][2 * int(path[j - 1] if j else path[0]) + int(path[j])]
            return tot

    def near(self, bound):
        """(the decisions of the recursion — a back-pointer of a step j >= 1, or the last state — whose exact margin is at most `bound`,
        the sum of those margins)"""
        n, loss = 0, 0.0
        for mg in [m_ for j, pair in enumerate(self.margin) if j for m_ in pair] + ([self.last_margin] if self.m else []):
            if mg <= bound:
                n += 1
                loss += float(mg)
        return n, loss


# ---------------------------------------------------------------------------------------------------------------- the device's order

def _mul(l, r):
    return (vmax(l[0] + r[0], l[1] + r[2]), vmax(l[0] + r[1], l[1] + r[3]), vmax(l[2] + r[0], l[3] + r[2]), vmax(l[2] + r[1], l[3] + r[3]))


def _vmul(x, m):
    s00, s10, s01, s11 = x[0] + m[0], x[1] + m[2], x[0] + m[1], x[1] + m[3]
    return (vmax(s00, s10), vmax(s01, s11)), (1 if s10 > s00 else 0) | (2 if s11 > s01 else 0)


_IDENTITY = (0.0, NINF, NINF, 0.0)


def _step(bwd, k, m, x, s, pi, q, length):
    if k >= m or (bwd and k == 0):
        return _IDENTITY
    l00, l01, l10, l11 = step(m - k if bwd else k, x, s, pi, q, length)
    return (l00, l10, l01, l11) if bwd else (l00, l01, l10, l11)


def _scan(bwd, x, s, pi, q, length):
    """the vectors and back-pointers after steps 0 .. m - 1 and the last carry, in the header's ORDER (hmm_ref._scan in the other algebra)"""
    m = len(s)
    T = H.threads(m)
    carry = (0.0, 0.0) if bwd else (math.log(q), math.log(pi))
    out, psi = [None] * m, [0] * m
    for k0 in range(0, m, T * CHUNK):
        live = min(T, -(-(m - k0) // CHUNK))
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
                v, _ = _vmul(v, prod[64 * w2 + 63])
            if l > 0:
                v, _ = _vmul(v, prod[t - 1])
            for c in range(CHUNK):
                k = k0 + t * CHUNK + c
                if k < m:
                    v, p = _vmul(v, steps[t][c])
                    out[k], psi[k] = v, p
            last = v
        carry = last
    return out, psi, carry


def viterbi_device_order(x, s, pi, length):
    """The decoding in the device's documented order -> dict(path, vit, delta)"""
    m = len(s)
    q = 1.0 - pi
    if m == 0:
        return dict(path=np.zeros(0, np.uint8), vit=0.0, delta=np.zeros(0))
    fw, psi, last = _scan(False, x, s, pi, q, length)
    bw, _, _ = _scan(True, x, s, pi, q, length)
    delta = np.array([(fw[j][1] + bw[m - 1 - j][1]) - (fw[j][0] + bw[m - 1 - j][0]) for j in range(m)])
    ups = [max(float(v), 0.0) for v in s]
    return dict(path=_traceback(psi, 1 if last[1] > last[0] else 0), vit=vmax(last[0], last[1]) + H._read_sum(ups, m), delta=delta)


# ---------------------------------------------------------------------------------------------------------------- counts, whole calls

def per_read(hoff, path):
    n = len(hoff) - 1
    res = {f: np.zeros(n, np.int32) for f in ('n_sites', 'n_mod', 'n_runs')}
    for r in range(n):
        st = np.asarray(path[hoff[r]:hoff[r + 1]])
        res['n_sites'][r] = len(st); res['n_mod'][r] = (st == 1).sum(); res['n_runs'][r] = len(H.runs(st)[0])
    return res


def per_site(site, path, nsites):
    site = np.asarray(site, np.int64)
    return dict(site_n=np.bincount(site, minlength=nsites).astype(np.int32),
                site_mod=np.bincount(site[np.asarray(path) == 1], minlength=nsites).astype(np.int32))


def read_viterbi_ref(cs, start, roff, score, key, pi, length, chain=viterbi_seq, exact=False):
    """Everything nmod_read_viterbi writes, from the restatement `chain` (viterbi_seq or viterbi_device_order), plus per read scale (D)
    and gate (G (D + 1)) and per row gate_row.  exact: also per read the MpChain (`mp`), opt (float), near, near_loss, and ref_delta /
    ref_path per row from mpmath"""
    hoff, site, x, s = H.entries_ref(cs, start, roff, score, key)
    n = len(hoff) - 1
    nrows = len(site)
    path, delta, g_row = np.zeros(nrows, np.uint8), np.zeros(nrows), np.zeros(nrows)
    vit, D, g = np.zeros(n), np.zeros(n), np.zeros(n)
    out = {}
    if exact:
        out.update(mp=[None] * n, opt=np.zeros(n), near=np.zeros(n, np.int64), near_loss=np.zeros(n), ref_delta=np.zeros(nrows), ref_path=np.zeros(nrows, np.uint8))
    for r in range(n):
        a, b = int(hoff[r]), int(hoff[r + 1])
        if b > a:
            res = chain(x[a:b], s[a:b], pi, length)
            path[a:b] = res['path']; delta[a:b] = res['delta']; vit[r] = res['vit']
            if exact:
                c = MpChain(x[a:b], s[a:b], pi, length)
                D[r] = c.scale
            else:
                D[r] = scale(x[a:b], s[a:b], pi, length)
            g[r] = gate(b - a) * (D[r] + 1.0)
            g_row[a:b] = g[r]
            if exact:
                out['mp'][r] = c; out['opt'][r] = float(c.opt); out['ref_delta'][a:b] = c.delta; out['ref_path'][a:b] = c.path
                out['near'][r], out['near_loss'][r] = c.near(g[r])
    out.update(hoff=hoff, site=site, x=x, s=s, path=path, delta=delta, vit=vit, scale=D, gate=g, gate_row=g_row,
               status=np.where(np.diff(hoff) == 0, NO_SITE, 0).astype(np.uint8))
    out.update(per_read(hoff, path))
    out.update(per_site(site, path, len(key)))
    return out


def excluded(ref):
    """per row: the reference's |delta| does not exceed its read's gate plus the read's near_loss (path equality says nothing there)"""
    loss = np.repeat(ref['near_loss'], np.diff(ref['hoff']))
    return np.abs(ref['ref_delta']) <= ref['gate_row'] + loss


def half_scores(m, s, first_positive=True):
    """+s on the first half and -s on the second (or the mirror image): the tie fixture of pi = 0.5"""
    v = np.full(m, -float(s))
    v[:m // 2] = float(s)
    return v if first_positive else -v
