"""The definitions of nmod_read_hmm_prior, nmod_read_viterbi_prior and nmod_read_hmm_grad_prior (include/nanomod_hip.h, K23) restated
from the header's text: K19's, K20's and K21's chain with a share per entry.  `p` below is always the RESOLVED share of every entry
(resolve(): site_pi at the entry's site, opts->pi where that word is a NaN, clamped to 1e-9 .. 1 - 1e-9) and q_j = 1.0 - p_j the double
the device forms.  Per algebra: a sequential float64 restatement, a 60-digit mpmath one, one in the device's documented order (built on
hmm_ref's _mul, _vmul, _wave_sum, _read_sum, on viterbi_ref's _mul, _vmul, _traceback and on hmm_fit_ref's _terms), and a brute force
over all 2^m paths that shares no code with any scan.  Nothing here calls the library.

THE GATES are those of hmm_ref, viterbi_ref and hmm_fit_ref: rounding counts per step, derived there.  What the prior form adds:
  K19 / K21  one subtraction per entry, q_j = 1 - p_j.  The plain form made the same subtraction once on the host with the same rounding,
             and both mpmath restatements take q as the double that results: nothing is added.  G = hmm_ref.gate, and the transition's
             bound ARG_U holds per entry (it is a bound over all allowed pi).
  K20        log p_j and log q_j come from the device's logarithm (within 1 ulp = 2 u of their size) where the plain form took the
             host's.  Inside a step they are what viterbi_ref's STEP_REL already counts at the device's bound (the rounding of
             log pi + log eps is counted as 2 u |log(pi eps)|): nothing is added per step.  The initial law (log q_0, log p_0) was the
             host's, correctly rounded, and viterbi_ref counts no rounding for it; here it carries 2 u of its size, at most 2 u D: TWO
             more roundings of size u D per pass, and forward and backward double it as everything else:
                 G_V(m) = min(CAP, u (2 (38 + 4 + 2 + tiles PATH_V(W)) + SUM_V + 6)).
             D is viterbi_ref's scale with the entry's own shares: max(|log q_0|, |log p_0|) + sum_j max |L_j| + sum_j max(s_j, 0).
  g_eta      the term of transition j is (p_j q_j) P_j: the product p_j q_j stands where the host's pi q stood, and the product with P_j
             is made once per term where the plain form made it once on the sum: ONE more relative rounding of every term, 1 u abs_eta:
                 G_ETA_P(m) = min(CAP, u (REL_U + 1 + VEC_U + m + 7 + (m - 1) (VEC_U + 3) + 2 VEC_U + 5)).
             hmm_fit_ref's bound p q M_j <= max(p, q) < 1 holds with the entry's own share.  g_lam keeps hmm_fit_ref.gate_lam."""
import math

import numpy as np

import hmm_fit_ref as F
import hmm_ref as H
import viterbi_ref as V

U, CAP, CHUNK = H.U, H.CAP, H.CHUNK
PI_LO, PI_HI = 1e-9, 1.0 - 1e-9
NINF = -math.inf

gate = H.gate
gate_lam = F.gate_lam


def gate_vit(m):
    T = H.threads(m)
    tiles = -(-m // (T * CHUNK))
    return min(V.CAP, U * (2 * (V.STEP_U + V.STEP_REL + 2 + tiles * V.path_v(T // 64)) + (CHUNK * tiles + 8 + T // 64) + 6))


def gate_eta(m):
    v = F.vec_u(m)
    return min(CAP, U * (F.REL_U + 1 + v + m + 7 + (m - 1) * (v + 3) + 2 * v + 5))


def resolve(site_pi, site, pi):
    """the share of every entry: site_pi[site_j], pi where that word is a NaN, clamped (an infinity with the rest)"""
    p = np.asarray(site_pi, np.float64)[np.asarray(site, np.int64)]
    p = np.where(np.isnan(p), float(pi), p)
    return np.minimum(np.maximum(p, PI_LO), PI_HI)


def transition(d, pj, length):
    """T_j with the share of the entry arrived at, K19's operations"""
    q = 1.0 - pj
    r = d / length
    rho, eps = math.exp(-r), -math.expm1(-r)
    return q + pj * rho, pj * eps, q * eps, pj + q * rho


# ---------------------------------------------------------------------------------------------------------------- sequential float64

def hmm_seq(x, s, p, length):
    """hmm_ref.hmm_seq with a share per entry -> dict(post, ll, ll_indep, denom)"""
    m = len(s)
    if m == 0:
        return dict(post=np.zeros(0), ll=0.0, ll_indep=0.0, denom=0.0)
    al = np.zeros((m, 2))
    ll = ind = denom = 0.0
    a0, a1 = 1.0 - float(p[0]), float(p[0])
    for j in range(m):
        pj = float(p[j])
        qj = 1.0 - pj
        e0, e1 = H.emission(float(s[j]))
        if j:
            t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), pj, length)
            a0, a1 = a0 * t00 + a1 * t10, a0 * t01 + a1 * t11
        a0, a1 = a0 * e0, a1 * e1
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        al[j] = a0, a1
        up = max(float(s[j]), 0.0)
        ll += math.log(c) + up
        ind += math.log(qj * e0 + pj * e1) + up
        denom += abs(math.log(c)) + up
    post = np.zeros(m)
    b0 = b1 = 1.0
    for j in range(m - 1, -1, -1):
        p0, p1 = al[j, 0] * b0, al[j, 1] * b1
        post[j] = p1 / (p0 + p1)
        if j:
            e0, e1 = H.emission(float(s[j]))
            t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), float(p[j]), length)
            y0, y1 = e0 * b0, e1 * b1
            b0, b1 = t00 * y0 + t01 * y1, t10 * y0 + t11 * y1
            c = b0 + b1
            b0, b1 = b0 / c, b1 / c
    return dict(post=post, ll=ll, ll_indep=ind, denom=denom, alpha=al)


def grad_seq(x, s, p, length):
    """hmm_fit_ref.grad_seq with a share per entry: g_eta = (post_0 - p_0) + SUM (p_j q_j) P_j, the product rounded, then added"""
    m = len(s)
    if m == 0:
        return dict(F.ZERO)
    fw = hmm_seq(x, s, p, length)
    al = fw['alpha']
    sp = sl = ap = alam = 0.0
    b0 = b1 = 1.0
    for j in range(m - 1, 0, -1):
        pj = float(p[j])
        qj = 1.0 - pj
        e0, e1 = H.emission(float(s[j]))
        r = float(x[j] - x[j - 1]) / length
        rho, eps = math.exp(-r), -math.expm1(-r)
        t = (qj + pj * rho, pj * eps, qj * eps, pj + qj * rho)
        y0, y1 = e0 * b0, e1 * b1
        pt, lt = F._terms(al[j - 1], (y0, y1), t, pj, qj, rho, eps, r)
        pt = (pj * qj) * pt
        sp += pt; sl += lt; ap += abs(pt); alam += abs(lt)
        b0, b1 = t[0] * y0 + t[1] * y1, t[2] * y0 + t[3] * y1
        c = b0 + b1
        b0, b1 = b0 / c, b1 / c
    p0, p1 = al[0, 0] * b0, al[0, 1] * b1
    first = p1 / (p0 + p1) - float(p[0])
    return dict(ll=fw['ll'], g_eta=first + sp, g_lam=sl, abs_eta=abs(first) + ap, abs_lam=alam)


def vit_step(j, x, s, p, length):
    """L_j as (l00, l01, l10, l11): viterbi_ref.step with the entry's share and the logarithms of it"""
    le0, le1 = V.log_emission(float(s[j]))
    if j == 0:
        return le0, NINF, NINF, le1
    pj = float(p[j])
    qj = 1.0 - pj
    r = float(x[j] - x[j - 1]) / length
    rho, eps = math.exp(-r), -math.expm1(-r)
    leps = math.log(eps)
    return math.log(qj + pj * rho) + le0, (math.log(pj) + leps) + le1, (math.log(qj) + leps) + le0, math.log(pj + qj * rho) + le1


def vit_scale(x, s, p, length):
    d = max(abs(math.log(1.0 - float(p[0]))), abs(math.log(float(p[0]))))
    for j in range(len(s)):
        d += max(abs(v) for v in vit_step(j, x, s, p, length) if v != NINF) + max(float(s[j]), 0.0)
    return d


def viterbi_seq(x, s, p, length):
    """viterbi_ref.viterbi_seq with a share per entry -> dict(path, vit, delta)"""
    m = len(s)
    if m == 0:
        return dict(path=np.zeros(0, np.uint8), vit=0.0, delta=np.zeros(0))
    a = np.zeros((m, 2))
    psi = [0] * m
    a0, a1 = math.log(1.0 - float(p[0])), math.log(float(p[0]))
    for j in range(m):
        l00, l01, l10, l11 = vit_step(j, x, s, p, length)
        s00, s10, s01, s11 = a0 + l00, a1 + l10, a0 + l01, a1 + l11
        psi[j] = (1 if s10 > s00 else 0) | (2 if s11 > s01 else 0)
        a0, a1 = V.vmax(s00, s10), V.vmax(s01, s11)
        a[j] = a0, a1
    b = np.zeros((m, 2))
    b0 = b1 = 0.0
    for j in range(m - 1, 0, -1):
        l00, l01, l10, l11 = vit_step(j, x, s, p, length)
        b0, b1 = V.vmax(b0 + l00, b1 + l01), V.vmax(b0 + l10, b1 + l11)
        b[j - 1] = b0, b1
    up = 0.0
    for v in s:
        up += max(float(v), 0.0)
    return dict(path=V._traceback(psi, 1 if a[m - 1, 1] > a[m - 1, 0] else 0), vit=V.vmax(a[m - 1, 0], a[m - 1, 1]) + up,
                delta=(a[:, 1] + b[:, 1]) - (a[:, 0] + b[:, 0]))


# ---------------------------------------------------------------------------------------------------------------- mpmath

def _mp_chain(x, s, p, q, L):
    """emissions and transitions as mpf from mpf shares (call inside mp.workdps): E[j], T[j], R[j] = (rho, eps, r)"""
    import mpmath as mp
    zero = mp.mpf(0)
    E, T, R = [], [None], [None]
    for j in range(len(s)):
        sj = mp.mpf(float(s[j]))
        E.append((mp.exp(-max(sj, zero)), mp.exp(min(sj, zero))))
        if j:
            r = mp.mpf(float(x[j] - x[j - 1])) / L
            rho, eps = mp.exp(-r), -mp.expm1(-r)
            T.append((q[j] + p[j] * rho, p[j] * eps, q[j] * eps, p[j] + q[j] * rho))
            R.append((rho, eps, r))
    return E, T, R


def ll_mp(x, s, p, q, L):
    """the chain's ll from mpf shares p, q and an mpf length (call inside mp.workdps): what the central differences need"""
    import mpmath as mp
    zero = mp.mpf(0)
    E, T, _ = _mp_chain(x, s, p, q, L)
    a0, a1 = q[0], p[0]
    ll = zero
    for j in range(len(s)):
        if j:
            t = T[j]
            a0, a1 = a0 * t[0] + a1 * t[2], a0 * t[1] + a1 * t[3]
        a0, a1 = a0 * E[j][0], a1 * E[j][1]
        c = a0 + a1
        a0, a1 = a0 / c, a1 / c
        ll += mp.log(c) + max(mp.mpf(float(s[j])), zero)
    return ll


def chain_mp(x, s, p, length, dps=60):
    """posterior, ll, ll_indep, denom and the gradient at `dps` digits, p, length, x, s taken as the exact doubles they are and q_j as
    the double 1.0 - p_j -> dict of mpf (post a list)"""
    import mpmath as mp
    with mp.workdps(dps):
        m = len(s)
        zero, one = mp.mpf(0), mp.mpf(1)
        if m == 0:
            return dict(post=[], ll=zero, ll_indep=zero, denom=zero, g_eta=zero, g_lam=zero, abs_eta=zero, abs_lam=zero)
        pm = [mp.mpf(float(v)) for v in p]
        qm = [mp.mpf(1.0 - float(v)) for v in p]
        L = mp.mpf(float(length))
        E, T, R = _mp_chain(x, s, pm, qm, L)
        al, ll, ind, denom = [], zero, zero, zero
        a0, a1 = qm[0], pm[0]
        for j in range(m):
            if j:
                t = T[j]
                a0, a1 = a0 * t[0] + a1 * t[2], a0 * t[1] + a1 * t[3]
            a0, a1 = a0 * E[j][0], a1 * E[j][1]
            c = a0 + a1
            a0, a1 = a0 / c, a1 / c
            al.append((a0, a1))
            up = max(mp.mpf(float(s[j])), zero)
            ll += mp.log(c) + up
            ind += mp.log(qm[j] * E[j][0] + pm[j] * E[j][1]) + up
            denom += abs(mp.log(c)) + up
        post = [zero] * m
        sp = sl = ap = alam = zero
        b0 = b1 = one
        for j in range(m - 1, -1, -1):
            p0, p1 = al[j][0] * b0, al[j][1] * b1
            post[j] = p1 / (p0 + p1)
            if j:
                t = T[j]
                rho, eps, r = R[j]
                y0, y1 = E[j][0] * b0, E[j][1] * b1
                pt, lt = F._terms(al[j - 1], (y0, y1), t, pm[j], qm[j], rho, eps, r)
                pt = pm[j] * qm[j] * pt
                sp += pt; sl += lt; ap += abs(pt); alam += abs(lt)
                b0, b1 = t[0] * y0 + t[1] * y1, t[2] * y0 + t[3] * y1
                c = b0 + b1
                b0, b1 = b0 / c, b1 / c
        first = post[0] - pm[0]
        return dict(post=post, ll=ll, ll_indep=ind, denom=denom, g_eta=first + sp, g_lam=sl, abs_eta=abs(first) + ap, abs_lam=alam)


def viterbi_mp(x, s, p, length, gate_abs=0.0, dps=60):
    """the decoding at `dps` digits -> dict(path, vit (mpf), delta (float64), scale, near_loss): near_loss the sum of the exact margins
    of the decisions (back-pointers of j >= 1, the last state) within gate_abs, as viterbi_ref.MpChain.near gives it"""
    import mpmath as mp
    with mp.workdps(dps):
        m = len(s)
        zero, ninf = mp.mpf(0), mp.mpf('-inf')
        if m == 0:
            return dict(path=np.zeros(0, np.uint8), vit=zero, delta=np.zeros(0), scale=0.0, near_loss=0.0)
        pm = [mp.mpf(float(v)) for v in p]
        qm = [mp.mpf(1.0 - float(v)) for v in p]
        E, T, _ = _mp_chain(x, s, pm, qm, mp.mpf(float(length)))
        steps, up = [], zero
        for j in range(m):
            sj = mp.mpf(float(s[j]))
            le0, le1 = -max(sj, zero), min(sj, zero)
            up += max(sj, zero)
            steps.append((le0, ninf, ninf, le1) if j == 0 else (mp.log(T[j][0]) + le0, mp.log(T[j][1]) + le1, mp.log(T[j][2]) + le0, mp.log(T[j][3]) + le1))
        a0, a1 = mp.log(qm[0]), mp.log(pm[0])
        scale = max(abs(a0), abs(a1)) + sum((max(abs(v) for v in st if v != ninf) for st in steps), zero) + up
        a, psi, margins = [], [], []
        for j in range(m):
            l00, l01, l10, l11 = steps[j]
            s00, s10, s01, s11 = a0 + l00, a1 + l10, a0 + l01, a1 + l11
            psi.append((1 if s10 > s00 else 0) | (2 if s11 > s01 else 0))
            if j:
                margins += [abs(s10 - s00), abs(s11 - s01)]
            a0, a1 = max(s00, s10), max(s01, s11)
            a.append((a0, a1))
        margins.append(abs(a1 - a0))
        d = [None] * m
        d[m - 1] = float(a1 - a0)
        b0 = b1 = zero
        for j in range(m - 1, 0, -1):
            l00, l01, l10, l11 = steps[j]
            b0, b1 = max(b0 + l00, b1 + l01), max(b0 + l10, b1 + l11)
            d[j - 1] = float((a[j - 1][1] + b1) - (a[j - 1][0] + b0))
        return dict(path=V._traceback(psi, 1 if a1 > a0 else 0), vit=max(a0, a1) + up, delta=np.array(d), scale=float(scale),
                    near_loss=float(sum((v for v in margins if v <= gate_abs), zero)))


# ---------------------------------------------------------------------------------------------------------------- the device's order

def _scan(step_of, mul, vmul, carry, m):
    """hmm_ref._scan / viterbi_ref._scan for any step: the vectors (and what vmul returns beside them) after steps 0 .. m - 1 and the last
    carry, in the header's ORDER.  step_of(k): the matrix of step k; vmul(x, mat) -> (vector, extra)"""
    T = H.threads(m)
    out, extra = [None] * m, [0] * m
    for k0 in range(0, m, T * CHUNK):
        live = min(T, -(-(m - k0) // CHUNK))
        steps = [[step_of(k0 + t * CHUNK + c) for c in range(CHUNK)] for t in range(T)]
        prod = []
        for t in range(T):
            pr = steps[t][0]
            for c in range(1, CHUNK):
                pr = mul(pr, steps[t][c])
            prod.append(pr)
        for w in range(T // 64):
            lanes = prod[64 * w:64 * w + 64]
            for d in (1, 2, 4, 8, 16, 32):
                lanes = [mul(lanes[l - d], lanes[l]) if l >= d else lanes[l] for l in range(64)]
            prod[64 * w:64 * w + 64] = lanes
        last = None
        for t in sorted(set(range(live)) | {T - 1}):
            w, l = divmod(t, 64)
            v = carry
            for w2 in range(w):
                v, _ = vmul(v, prod[64 * w2 + 63])
            if l > 0:
                v, _ = vmul(v, prod[t - 1])
            for c in range(CHUNK):
                k = k0 + t * CHUNK + c
                if k < m:
                    v, e = vmul(v, steps[t][c])
                    out[k], extra[k] = v, e
            last = v
        carry = last
    return out, extra, carry


def _hmm_scans(x, s, p, length):
    m = len(s)

    def step_of(bwd):
        def f(k):
            if k >= m or (bwd and k == 0):
                return H._IDENTITY
            j = m - k if bwd else k
            e0, e1 = H.emission(float(s[j]))
            t00, t01, t10, t11 = transition(float(x[j] - x[j - 1]), float(p[j]), length) if j > 0 else (1.0, 0.0, 0.0, 1.0)
            return (e0 * t00, e0 * t10, e1 * t01, e1 * t11, 0) if bwd else (t00 * e0, t01 * e1, t10 * e0, t11 * e1, 0)
        return f
    vmul = lambda v, mat: (H._vmul(v, mat), 0)
    fw, _, last = _scan(step_of(False), H._mul, vmul, (1.0 - float(p[0]), float(p[0]), 0), m)
    bw, _, _ = _scan(step_of(True), H._mul, vmul, (1.0, 1.0, 0), m)
    return fw, bw, last


def hmm_device_order(x, s, p, length):
    """hmm_ref.hmm_device_order with a share per entry -> dict(post, ll, ll_indep)"""
    m = len(s)
    if m == 0:
        return dict(post=np.zeros(0), ll=0.0, ll_indep=0.0)
    fw, bw, last = _hmm_scans(x, s, p, length)
    post = np.zeros(m)
    for j in range(m):
        b = bw[m - 1 - j]
        p0, p1 = fw[j][0] * b[0], fw[j][1] * b[1]
        post[j] = p1 / (p0 + p1)
    ups = [max(float(v), 0.0) for v in s]
    ind = []
    for j in range(m):
        e0, e1 = H.emission(float(s[j]))
        pj = float(p[j])
        ind.append(math.log((1.0 - pj) * e0 + pj * e1) + ups[j])
    ll = (math.log(last[0] + last[1]) + float(last[2]) * H.LN2) + H._read_sum(ups, m)
    return dict(post=post, ll=ll, ll_indep=H._read_sum(ind, m))


def grad_device_order(x, s, p, length):
    """hmm_fit_ref.grad_device_order with a share per entry"""
    m = len(s)
    if m == 0:
        return dict(F.ZERO)
    fw, bw, last = _hmm_scans(x, s, p, length)
    tp, tl, tap, tal = ([0.0] * m for _ in range(4))
    for k in range(m - 1):
        j = m - 1 - k
        pj = float(p[j])
        qj = 1.0 - pj
        e0, e1 = H.emission(float(s[j]))
        r = float(x[j] - x[j - 1]) / length
        rho, eps = math.exp(-r), -math.expm1(-r)
        t = (qj + pj * rho, pj * eps, qj * eps, pj + qj * rho)
        pt, lt = F._terms(fw[j - 1], (e0 * bw[k][0], e1 * bw[k][1]), t, pj, qj, rho, eps, r)
        pt = (pj * qj) * pt
        tp[k], tl[k], tap[k], tal[k] = pt, lt, abs(pt), abs(lt)
    b = bw[m - 1]
    p0, p1 = fw[0][0] * b[0], fw[0][1] * b[1]
    first = p1 / (p0 + p1) - float(p[0])
    ll = (math.log(last[0] + last[1]) + float(last[2]) * H.LN2) + H._read_sum([max(float(v), 0.0) for v in s], m)
    return dict(ll=ll, g_eta=first + H._read_sum(tp, m), g_lam=H._read_sum(tl, m), abs_eta=abs(first) + H._read_sum(tap, m),
                abs_lam=H._read_sum(tal, m))


def viterbi_device_order(x, s, p, length):
    """viterbi_ref.viterbi_device_order with a share per entry -> dict(path, vit, delta)"""
    m = len(s)
    if m == 0:
        return dict(path=np.zeros(0, np.uint8), vit=0.0, delta=np.zeros(0))

    def step_of(bwd):
        def f(k):
            if k >= m or (bwd and k == 0):
                return V._IDENTITY
            l00, l01, l10, l11 = vit_step(m - k if bwd else k, x, s, p, length)
            return (l00, l10, l01, l11) if bwd else (l00, l01, l10, l11)
        return f
    fw, psi, last = _scan(step_of(False), V._mul, V._vmul, (math.log(1.0 - float(p[0])), math.log(float(p[0]))), m)
    bw, _, _ = _scan(step_of(True), V._mul, V._vmul, (0.0, 0.0), m)
    delta = np.array([(fw[j][1] + bw[m - 1 - j][1]) - (fw[j][0] + bw[m - 1 - j][0]) for j in range(m)])
    ups = [max(float(v), 0.0) for v in s]
    return dict(path=V._traceback(psi, 1 if last[1] > last[0] else 0), vit=V.vmax(last[0], last[1]) + H._read_sum(ups, m), delta=delta)


# ---------------------------------------------------------------------------------------------------------------- all paths

def brute_force(x, s, p, length):
    """Every one of the 2^m state paths (m <= 10) with its joint probability, in numpy and on the definition alone: no scan, no
    scaling, no code of the restatements above.  -> dict(post, ll, path (the first best in the order of the path's number), vit,
    delta): ll and vit on the header's scale (relative to `every site canonical`: S = sum max(s_j, 0) is added to the scaled emissions)"""
    m = len(s)
    assert 1 <= m <= 10
    x, s, p = np.asarray(x, np.float64), np.asarray(s, np.float64), np.asarray(p, np.float64)
    z = (np.arange(1 << m)[:, None] >> np.arange(m)[None, :]) & 1                   # [path, entry]
    logp = np.where(z[:, 0] == 1, np.log(p[0]), np.log1p(-p[0]))
    for j in range(m):
        logp = logp + np.where(z[:, j] == 1, np.minimum(s[j], 0.0), -np.maximum(s[j], 0.0))
        if j:
            keep = np.exp(-(x[j] - x[j - 1]) / length)
            law = np.where(z[:, j] == 1, p[j], 1.0 - p[j])                            # redraw from the site's own law
            logp = logp + np.log(keep * (z[:, j] == z[:, j - 1]) + (1.0 - keep) * law)
    S = float(np.maximum(s, 0.0).sum())
    top = logp.max()
    w = np.exp(logp - top)
    tot = w.sum()
    post = np.array([w[z[:, j] == 1].sum() / tot for j in range(m)])
    best = int(np.argmax(logp))
    delta = np.array([logp[z[:, j] == 1].max() - logp[z[:, j] == 0].max() for j in range(m)])
    return dict(post=post, ll=float(top + math.log(tot)) + S, path=z[best].astype(np.uint8), vit=float(top) + S, delta=delta,
                second=float(np.sort(logp)[-2]) + S if m else math.nan)


# ---------------------------------------------------------------------------------------------------------------- whole calls

def read_prior_ref(cs, start, roff, score, key, site_pi, pi, length, call_post, order=True):
    """Everything the three prior entries write, per read from the restatements (order: the device's order, else the sequential ones),
    with the gates: hmm_ref.read_hmm_ref's and viterbi_ref.read_viterbi_ref's keys (Viterbi's prefixed v_: v_path, v_delta, v_vit,
    v_gate per read = G_V (D + 1), v_gate_row) and hmm_fit_ref.read_grad_ref's (g_ll, g_eta, g_lam, abs_eta, abs_lam, gate_eta, gate_lam)"""
    hoff, site, x, s = H.entries_ref(cs, start, roff, score, key)
    p = resolve(site_pi, site, pi) if len(site) else np.zeros(0)
    n, nrows = len(hoff) - 1, len(site)
    post, g, path, delta, vg_row = np.zeros(nrows), np.zeros(nrows), np.zeros(nrows, np.uint8), np.zeros(nrows), np.zeros(nrows)
    per = {k: np.zeros(n) for k in ('ll', 'll_indep', 'denom', 'v_vit', 'v_gate', 'v_scale', 'g_ll', 'g_eta', 'g_lam', 'abs_eta', 'abs_lam',
                                    'gate_eta', 'gate_lam')}
    hmm, vit, grad = (hmm_device_order, viterbi_device_order, grad_device_order) if order else (hmm_seq, viterbi_seq, grad_seq)
    for r in range(n):
        a, b = int(hoff[r]), int(hoff[r + 1])
        if b == a:
            continue
        xs, ss, ps, m = x[a:b], s[a:b], p[a:b], b - a
        res = hmm(xs, ss, ps, length)
        post[a:b] = res['post']; per['ll'][r] = res['ll']; per['ll_indep'][r] = res['ll_indep']
        per['denom'][r] = hmm_seq(xs, ss, ps, length)['denom']
        g[a:b] = gate(m)
        res = vit(xs, ss, ps, length)
        path[a:b] = res['path']; delta[a:b] = res['delta']; per['v_vit'][r] = res['vit']
        per['v_scale'][r] = vit_scale(xs, ss, ps, length)
        per['v_gate'][r] = gate_vit(m) * (per['v_scale'][r] + 1.0)
        vg_row[a:b] = per['v_gate'][r]
        res = grad(xs, ss, ps, length)
        per['g_ll'][r] = res['ll']
        for k in ('g_eta', 'g_lam', 'abs_eta', 'abs_lam'):
            per[k][r] = res[k]
        per['gate_eta'][r], per['gate_lam'][r] = gate_eta(m), gate_lam(m)
    st = H.states(post, call_post)
    out = dict(hoff=hoff, site=site, x=x, s=s, p=p, post=post, state=st, gate=g, v_path=path, v_delta=delta, v_gate_row=vg_row,
               status=np.where(np.diff(hoff) == 0, H.NO_SITE, 0).astype(np.uint8), **per)
    out.update(H.per_read(hoff, st))
    out.update(H.per_site(site, st, len(key)))
    return out
