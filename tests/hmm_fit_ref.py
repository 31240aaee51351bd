"""The definition of nmod_read_hmm_grad (include/nanomod_hip.h, K21) restated from the header's text on top of hmm_ref (K19): the gradient
of a read's log-likelihood in eta = logit(pi) and lam = ln(length) from the sequential float64 chain, the same in 60-digit mpmath, the
same in the device's documented order, the fixed-order batch sums, a seeded simulator of chain reads, an evaluator for readllr.fit_hmm
built on the restatement, and the gates.  Nothing here calls the library.

THE GATES are derived, not tuned.  u = 2^-53, units as in hmm_ref.  With A = a_(j-1), y = e_j b_j and T = T_j the terms are
      P_j = eps (A0 + A1) (y1 - y0) / Z,     L_j = rho r (pi A0 - q A1) (y0 - y1) / Z,     Z = sum_rc A_r t_rc y_c.
  VEC_U(m) = STEP_U (m + 1) + 2 tiles PATH_U bounds the relative errors of a_(j-1) and b_j together (hmm_ref: forward and backward pass
  m + 1 step matrices between them); hmm_ref's gate of post is 2 VEC_U + 4.
  What multiplies a term, and so moves it by a relative amount:
      eps (its argument 1, expm1 EXP_U)                                                                                    3
      A0 + A1, the product with it, the product with the difference, the division                                         4
      Z: an entry of T (STEP_U less the emission's 3), y_c = e_jc b_jc (exp EXP_U, the product), two products and
         two sums per row and the last sum (counted once: the terms are non-negative, relative errors do not add up)      26 + 3 + 4
      the vectors                                                                                                          VEC_U
    = REL_U + VEC_U with REL_U = 40.  L_j has rho r for eps: r is rounded once (1), rho = exp(-r) moves by r u for that and by EXP_U,
    and r < 745 wherever rho is not 0; the product: LREL_U = REL_U + 745.
  What is subtracted, and so moves a term by an absolute amount: y1 - y0 is known to (VEC_U + 3) u (y0 + y1) (b, the emission and the
  product), which moves P_j by (VEC_U + 3) u M_j, M_j = eps (A0 + A1) (y0 + y1) / Z.  Every entry of T is at least eps min(pi, q)
  (t00 = q + pi rho >= q >= q eps, t11 likewise), so Z >= eps min(pi, q) (A0 + A1) (y0 + y1) and pi q M_j <= max(pi, q) < 1: per
  transition g_eta moves by at most (VEC_U + 3) u, whatever the parameters.  L_j has two differences, pi A0 - q A1 and y0 - y1, each
  known to (VEC_U + 3) u of the sum of its terms; N_j = rho r (pi A0 + q A1) (y0 + y1) / Z is bounded term by term against Z's four
  products by rho r / eps = r / (e^r - 1) <= 1 and r pi rho / (q + pi rho) = r / (1 + (q / pi) e^r) < 21 (hmm_ref's ARG_U argument; the
  same with pi and q exchanged), so N_j <= ARG_U: per transition g_lam moves by at most 2 ARG_U (VEC_U + 3) u.
  The first entry: post_0 is known to hmm_ref's gate relative to itself, at most 1, and post_0 - pi adds one rounding: 2 VEC_U + 5.
  The sums: m values of one sign at worst in abs, each addition u of the partial sum, the wave sum 7 deep: less than (m + 7) u of abs.
  With abs_eta = |post_0 - pi| + pi q sum |P_j| and abs_lam = sum |L_j|:
      |g_eta - ref| <= u ((REL_U + VEC_U + m + 7) abs_eta + (m - 1) (VEC_U + 3) + 2 VEC_U + 5)
      |g_lam - ref| <= u ((LREL_U + VEC_U + m + 7) abs_lam + 2 ARG_U (m - 1) (VEC_U + 3))
  and, both being at most their sum times (abs + 1),
      G_ETA(m) = min(CAP, u (REL_U + VEC_U + m + 7 + (m - 1) (VEC_U + 3) + 2 VEC_U + 5)),        |g_eta - ref| <= G_ETA (abs_eta + 1),
      G_LAM(m) = min(CAP, u (LREL_U + VEC_U + m + 7 + 2 ARG_U (m - 1) (VEC_U + 3))),             |g_lam - ref| <= G_LAM (abs_lam + 1).
  CAP = hmm_ref's 1e-12, for hmm_ref's reason: the chain forgets, the errors of the vectors do not in fact grow with m and those of
  the terms do not all point one way, and a gate that grew as m^2 would hide a wrong carry or a term taken twice.  It binds from
  m = 16 (G_ETA) and m = 3 (G_LAM).  The 1: a read whose terms cancel (every score 0: y1 - y0 is rounding alone) has abs near 0
  and a g that no order of double operations gives as an exact 0.
  ll is not gated: it is nmod_read_hmm's, bit for bit."""
import math

import numpy as np

import hmm_ref as H

U, CAP = H.U, H.CAP
REL_U = 40
LREL_U = REL_U + 745
PI_RANGE, LENGTH_RANGE = (1e-9, 1.0 - 1e-9), (1e-3, 1e9)
SUM_THREADS = 256


def vec_u(m):
    T = H.threads(m)
    tiles = -(-m // (T * H.CHUNK))
    return H.STEP_U * (m + 1) + 2 * tiles * H.path_u(T // 64)


def gate_eta(m):
    v = vec_u(m)
    return min(CAP, U * (REL_U + v + m + 7 + (m - 1) * (v + 3) + 2 * v + 5))


def gate_lam(m):
    v = vec_u(m)
    return min(CAP, U * (LREL_U + v + m + 7 + 2 * H.ARG_U * (m - 1) * (v + 3)))


def within(got, ref, g, scale):
    """|got - ref| <= g (scale + 1), elementwise (scale: abs_eta or abs_lam of the reference)"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) <= np.asarray(g) * (np.asarray(scale, np.float64) + 1.0)


ZERO = dict(ll=0.0, g_eta=0.0, g_lam=0.0, abs_eta=0.0, abs_lam=0.0)


# ---------------------------------------------------------------------------------------------------------------- the sequential chain

def _terms(A, y, t, pi, q, rho, eps, r):
    """P_j and L_j as the header writes them, left to right"""
    z = A[0] * (t[0] * y[0] + t[1] * y[1]) + A[1] * (t[2] * y[0] + t[3] * y[1])
    return eps * (A[0] + A[1]) * (y[1] - y[0]) / z, rho * r * (pi * A[0] - q * A[1]) * (y[0] - y[1]) / z


def grad_seq(x, s, pi, length):
    """ll and its gradient from the sequential scaled forward-backward of hmm_ref.hmm_seq -> dict(ll, g_eta, g_lam, abs_eta, abs_lam)"""
    m = len(s)
    if m == 0:
        return dict(ZERO)
    q = 1.0 - pi
    al = np.zeros((m, 2))
    a0, a1 = q, pi
    ll = 0.0
    for j in range(m):
        e0, e1 = H.emission(float(s[j]))
        if j:
            t00, t01, t10, t11 = H.transition(float(x[j] - x[j - 1]), pi, q, length)
            a0, a1 = a0 * t00 + a1 * t10, a0 * t01 + a1 * t11
        a0, a1 = a0 * e0, a1 * e1
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        al[j] = a0, a1
        ll += math.log(c) + max(float(s[j]), 0.0)
    sp = sl = ap = alam = 0.0
    b0 = b1 = 1.0
    for j in range(m - 1, 0, -1):
        e0, e1 = H.emission(float(s[j]))
        r = float(x[j] - x[j - 1]) / length
        rho, eps = math.exp(-r), -math.expm1(-r)
        t = (q + pi * rho, pi * eps, q * eps, pi + q * rho)
        y0, y1 = e0 * b0, e1 * b1
        p, l = _terms(al[j - 1], (y0, y1), t, pi, q, rho, eps, r)
        sp += p; sl += l; ap += abs(p); alam += abs(l)
        b0, b1 = t[0] * y0 + t[1] * y1, t[2] * y0 + t[3] * y1
        c = b0 + b1
        b0, b1 = b0 / c, b1 / c
    p0, p1 = al[0, 0] * b0, al[0, 1] * b1
    first = p1 / (p0 + p1) - pi
    return dict(ll=ll, g_eta=first + pi * q * sp, g_lam=sl, abs_eta=abs(first) + pi * q * ap, abs_lam=alam)


# ---------------------------------------------------------------------------------------------------------------- mpmath

def ll_mp(x, s, pi, q, length):
    """hmm_ref.hmm_mp's ll with pi, q and length as mpf (call inside mp.workdps): what its central differences need, since hmm_mp takes
    its parameters as doubles.  At the doubles (pi, 1.0 - pi, length) it is hmm_mp's ll"""
    import mpmath as mp
    zero = mp.mpf(0)
    a0, a1 = q, pi
    ll = zero
    for j in range(len(s)):
        sj = mp.mpf(float(s[j]))
        e0, e1 = mp.exp(-max(sj, zero)), mp.exp(min(sj, zero))
        if j:
            r = mp.mpf(float(x[j] - x[j - 1])) / length
            rho, eps = mp.exp(-r), -mp.expm1(-r)
            a0, a1 = a0 * (q + pi * rho) + a1 * (q * eps), a0 * (pi * eps) + a1 * (pi + q * rho)
        a0, a1 = a0 * e0, a1 * e1
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        ll += mp.log(c) + max(sj, zero)
    return ll


def grad_mp(x, s, pi, length, dps=60):
    """the header's definition in mpmath at `dps` digits, pi, length, x and s taken as the exact doubles they are and q as the double
    1.0 - pi the entry forms -> dict of mpf"""
    import mpmath as mp
    with mp.workdps(dps):
        m = len(s)
        zero, one = mp.mpf(0), mp.mpf(1)
        if m == 0:
            return {k: zero for k in ZERO}
        pi_, L = mp.mpf(float(pi)), mp.mpf(float(length))
        q = mp.mpf(1.0 - float(pi))
        E, T, R = [], [None], [None]
        for j in range(m):
            sj = mp.mpf(float(s[j]))
            E.append((mp.exp(-max(sj, zero)), mp.exp(min(sj, zero))))
            if j:
                r = mp.mpf(float(x[j] - x[j - 1])) / L
                rho, eps = mp.exp(-r), -mp.expm1(-r)
                T.append((q + pi_ * rho, pi_ * eps, q * eps, pi_ + q * rho))
                R.append((rho, eps, r))
        al, ll = [], zero
        a0, a1 = q, pi_
        for j in range(m):
            if j:
                t = T[j]
                a0, a1 = a0 * t[0] + a1 * t[2], a0 * t[1] + a1 * t[3]
            a0, a1 = a0 * E[j][0], a1 * E[j][1]
            c = a0 + a1
            a0, a1 = a0 / c, a1 / c
            al.append((a0, a1))
            ll += mp.log(c) + max(mp.mpf(float(s[j])), zero)
        sp = sl = ap = alam = zero
        b0 = b1 = one
        for j in range(m - 1, 0, -1):
            t = T[j]
            rho, eps, r = R[j]
            y0, y1 = E[j][0] * b0, E[j][1] * b1
            p, l = _terms(al[j - 1], (y0, y1), t, pi_, q, rho, eps, r)
            sp += p; sl += l; ap += abs(p); alam += abs(l)
            b0, b1 = t[0] * y0 + t[1] * y1, t[2] * y0 + t[3] * y1
            c = b0 + b1
            b0, b1 = b0 / c, b1 / c
        p0, p1 = al[0][0] * b0, al[0][1] * b1
        first = p1 / (p0 + p1) - pi_
        return dict(ll=ll, g_eta=first + pi_ * q * sp, g_lam=sl, abs_eta=abs(first) + pi_ * q * ap, abs_lam=alam)


# ---------------------------------------------------------------------------------------------------------------- the device's order

def grad_device_order(x, s, pi, length):
    """The same in the device's documented order: hmm_ref's two scans, the term of transition j formed at backward step m - 1 - j, a
    thread's terms added in the order of its steps, the wave sum, the waves in order (hmm_ref._read_sum over the steps)"""
    m = len(s)
    if m == 0:
        return dict(ZERO)
    q = 1.0 - pi
    fw, last = H._scan(False, x, s, pi, q, length)
    bw, _ = H._scan(True, x, s, pi, q, length)
    tp, tl, tap, tal = ([0.0] * m for _ in range(4))
    for k in range(m - 1):
        j = m - 1 - k
        e0, e1 = H.emission(float(s[j]))
        r = float(x[j] - x[j - 1]) / length
        rho, eps = math.exp(-r), -math.expm1(-r)
        t = (q + pi * rho, pi * eps, q * eps, pi + q * rho)
        p, l = _terms(fw[j - 1], (e0 * bw[k][0], e1 * bw[k][1]), t, pi, q, rho, eps, r)
        tp[k], tl[k], tap[k], tal[k] = p, l, abs(p), abs(l)
    b = bw[m - 1]
    p0, p1 = fw[0][0] * b[0], fw[0][1] * b[1]
    first = p1 / (p0 + p1) - pi
    ll = (math.log(last[0] + last[1]) + float(last[2]) * H.LN2) + H._read_sum([max(float(v), 0.0) for v in s], m)
    return dict(ll=ll, g_eta=first + (pi * q) * H._read_sum(tp, m), g_lam=H._read_sum(tl, m), abs_eta=abs(first) + (pi * q) * H._read_sum(tap, m),
                abs_lam=H._read_sum(tal, m))


# ---------------------------------------------------------------------------------------------------------------- the batch

def _block_sum(v):
    """one word over the reads: thread t adds reads t, t + 256, ... in ascending order, the wave sums, the four waves in order"""
    v = np.asarray(v, np.float64)
    per = np.zeros(SUM_THREADS)
    for r0 in range(0, len(v), SUM_THREADS):
        part = v[r0:r0 + SUM_THREADS]
        per[:len(part)] = per[:len(part)] + part
    tot = np.float64(0.0)
    for w in range(SUM_THREADS // 64):
        tot = tot + H._wave_sum(per[64 * w:64 * w + 64])
    return float(tot)


def batch_sums(ll, g_eta, g_lam, hoff):
    """the eight words of `sums` from the per-read values, in the header's order (a product is rounded, then added)"""
    ll, e, v = (np.asarray(a, np.float64) for a in (ll, g_eta, g_lam))
    m = np.diff(np.asarray(hoff, np.int64))
    return np.array([_block_sum(a) for a in (ll, e, v, e * e, e * v, v * v, (m > 0).astype(np.float64), np.maximum(m, 0).astype(np.float64))])


def read_grad_ref(cs, start, roff, score, key, pi, length, chain=grad_seq):
    """Everything nmod_read_hmm_grad writes per read, from the restatement `chain`, plus hoff, x, s and the gates per read"""
    hoff, site, x, s = H.entries_ref(cs, start, roff, score, key)
    n = len(hoff) - 1
    out = {k: np.zeros(n) for k in ZERO}
    for r in range(n):
        a, b = int(hoff[r]), int(hoff[r + 1])
        res = chain(x[a:b], s[a:b], pi, length)
        for k in ZERO:
            out[k][r] = float(res[k])
    m = np.diff(hoff)
    out.update(hoff=hoff, x=x, s=s, status=np.where(m == 0, H.NO_SITE, 0).astype(np.uint8),
               gate_eta=np.array([gate_eta(int(v)) if v else 0.0 for v in m]), gate_lam=np.array([gate_lam(int(v)) if v else 0.0 for v in m]))
    return out


# ---------------------------------------------------------------------------------------------------------------- simulated reads

def simulate_chain_reads(seed=2103, n_reads=300, pi=0.3, length=150.0, sep=2.0, entries=(5, 25), gaps=(1, 23)):
    """Reads drawn from the model itself: per read m in entries[0] .. entries[1] sites at gaps of gaps[0] .. gaps[1] bases, the states a
    chain with the stationary share pi and correlation exp(-d / length), the score of an entry the log-likelihood ratio of two
    unit-variance normals `sep` apart, sep z - sep^2 / 2 with z ~ N(sep state, 1).  A list of (x, s) float64 arrays"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        m = int(rng.integers(entries[0], entries[1] + 1))
        x = np.concatenate(([0], np.cumsum(rng.integers(gaps[0], gaps[1] + 1, m - 1)))).astype(np.float64) if m > 0 else np.zeros(0)
        z = np.zeros(m, np.int64)
        for j in range(m):
            if j == 0:
                p1 = pi
            else:
                rho = math.exp(-(x[j] - x[j - 1]) / length)
                p1 = pi + (1.0 - pi) * rho if z[j - 1] else pi * (1.0 - rho)
            z[j] = rng.random() < p1
        obs = rng.normal(sep * z, 1.0)
        reads.append((x, sep * obs - 0.5 * sep * sep))
    return reads


def walk_inputs(reads):
    """the reads of simulate_chain_reads as nmod_read_hmm's arguments: one '+' chromosome whose every position is a candidate site, a read
    from position 0 with a NaN score wherever it has no entry -> dict(cs, start, roff, score, key)"""
    top = max([int(x[-1]) + 1 for x, _ in reads if len(x)] + [1])
    score, roff = [], [0]
    for x, s in reads:
        row = np.full(int(x[-1]) + 1 if len(x) else 1, np.nan)
        row[x.astype(np.int64)] = s
        score.append(row)
        roff.append(roff[-1] + len(row))
    return dict(cs=np.zeros(len(reads), np.int32), start=np.zeros(len(reads), np.int64), roff=np.array(roff, np.int64),
                score=np.concatenate(score) if score else np.zeros(0), key=np.arange(top, dtype=np.int64))


def evaluator(reads, chain=grad_seq):
    """evaluate(pi, length) for readllr.fit_hmm from the restatement: the fixed-order sums of the per-read values"""
    hoff = np.concatenate(([0], np.cumsum([len(s) for _, s in reads]))).astype(np.int64)

    def evaluate(pi, length):
        res = [chain(x, s, pi, length) for x, s in reads]
        return batch_sums([r['ll'] for r in res], [r['g_eta'] for r in res], [r['g_lam'] for r in res], hoff).tolist()
    return evaluate
