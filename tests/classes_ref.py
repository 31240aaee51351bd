"""The definition of nmod_read_class_rows / nmod_read_classes_step (include/nanomod_hip.h, K22) restated from the header's text, in
three parts: (a) step_ref, sequential float64 in the device's documented order of operations; (b) step_mp, the same step in mpmath
with the gates; (c) em_ref, the loop.  Beside them step_vec (the step vectorised, any order: what the loop runs on), step_dense (every
read x site x class with masks), the rows of a sample and the planted sample.  Nothing here calls the library.

THE GATES are derived, not tuned.  u = 2^-53.  EXP_U = 2: exp, expm1, log and log1p of the device's double-precision library are within
1 ulp = 2 u, the constant tests/hmm_ref.py takes for the same functions.  To first order:
  an entry's term g = log1p(-x), x = f t, f = 1 - th or th, t = -expm1(-|s|):
      f one rounding (none for th), t EXP_U, the product one: x is known to X_U = 4 u relatively.  d/dx log1p(-x) = -1 / (1 - x), so
      the term moves by X_U u x / (1 - x), and the library's log1p adds EXP_U u |g|.  x / (1 - x) is about |g| for a moderate x and
      grows beyond it as x nears 1, which a share at a clamp and a score beyond +-37 (t rounds to 1) reach: 1 - x is then the 1e-9 of
      the clamp, formed from doubles that are known to u only.  That amplification is the definition's (it forms 1 - (1 - th) t), not an
      order of operations', so the gate carries it as AMP = sum_j x_j / (1 - x_j) beside ABSG = sum_j |g_j|.
  l_rc, a sum of m terms by T threads: a term passes ceil(m / T) additions of its thread, eight of the wave sum and four of the waves:
      SUM_U(m, T) = ceil(m / T) + 12 roundings relative to ABSG.
  a_rc = log w_c + l_rc: EXP_U + 1 on |log w_c|, one more on |a_rc| <= |log w_c| + ABSG.  So
      G_A(r, c) = u (X_U AMP + (EXP_U + SUM_U + 1) ABSG + (EXP_U + 2) |log w_c|).
  ll_r = (M + log Z) + S: M is one of the a; x_c = exp(a_c - M) is known to G_A(c) + G_A(cM) + u |a_c - M| + EXP_U u relatively, and
      x_c |a_c - M| <= 1 / e; Z in [1, C] adds C roundings, log Z EXP_U on at most ln 8, the two additions two roundings on
      |M| + ln C + S, and S is a sum like l: so, with D = max_c ABSG + S + 1 (what the issue asks ll to be relative to),
      G_LL(r) = 3 max_c G_A(r, c) + u ((SUM_U + 3) (S + max_c |a_c|) + 2 EXP_U + C + 4).
  gamma_rc = x_c / Z, an absolute gate: the relative errors of x_c and of Z, times gamma <= 1, and the division:
      G_GAMMA(r) = 4 max_c G_A(r, c) + (2 EXP_U + C + 2) u.
  post(s, th).  s >= 0: th / (1 - x): the denominator moves by X_U u x + u (1 - x), the division adds one:
      post (X_U x / (1 - x) + 2) u.  s < 0: th (1 - t) / (1 - th t): 1 - t is known to EXP_U u t + u absolutely, so the numerator to
      (EXP_U + 2) u th; the denominator d as before with x = th t.  Together G_POST = u ((EXP_U + 2) th / d [s < 0] + post (X_U x / d + 2)).
  N_jc = sum gamma and Mo_jc = sum gamma post over the n rows of a site by G threads: SUM_U(n, G) roundings relative to the sums, a
      product's own rounding, and the errors of the factors:
      G_N = sum_rows G_GAMMA + SUM_U u N,   G_MO = sum_rows (gamma G_POST + post G_GAMMA + u gamma post) + SUM_U u Mo.
  theta_out = Mo / N moves by (G_MO + theta G_N) / N + u theta: it is compared relative to N, as
      |theta_out - ref| N <= G_MO + theta G_N + u theta N =: G_THETA   (the clamp to 1e-9 .. 1 - 1e-9 brings two values no further apart).
  A class that no read prefers has gamma = 0 exactly on the device (exp underflows) and 1e-400 here: N is 0 there and theta_out stays
  theta_in, which the gate relative to N accepts: |theta_in - ref| N is far below sum_rows G_GAMMA.
cls is the arg max of gamma: it is compared where the two largest gamma of this file's mpmath step differ by more than 2 G_GAMMA."""
import math

import numpy as np

import hmm_ref as H

U = H.U
EXP_U = H.EXP_U
X_U = 4
CLASSES_MAX, SMALL, WAVE = 8, 64, 512                # NMOD_CLASSES_MAX, NMOD_CLASSES_SMALL, NMOD_CLASSES_WAVE; test_read_classes.py checks them
WAVE_MAX = H.WAVE_MAX                                # NMOD_HMM_WAVE_MAX
NO_SITE = H.NO_SITE
LO, HI = 1e-9, 1.0 - 1e-9
DBL_MAX = H.DBL_MAX
SUMS = 4                                             # words of `sums` in front of the classes'


def read_threads(m):
    return 64 if m <= WAVE_MAX else 256


def site_threads(n):
    return 16 if n <= SMALL else (64 if n <= WAVE else 256)


def sum_u(n, threads):
    return -(-n // threads) + 12


# ---------------------------------------------------------------------------------------------------------------- the rows

def rows_from_entries(hoff, site, s, nsites):
    """nmod_read_class_rows' outputs from the entries of the reads: dict(hoff, site, s, rread, soff, srow)"""
    hoff = np.asarray(hoff, np.int64)
    site = np.asarray(site, np.int32)
    rread = np.repeat(np.arange(len(hoff) - 1, dtype=np.int32), np.diff(hoff))
    soff = np.zeros(nsites + 1, np.int64)
    soff[1:] = np.cumsum(np.bincount(site, minlength=nsites))
    return dict(hoff=hoff, site=site, s=np.asarray(s, np.float64), rread=rread, soff=soff, srow=np.argsort(site, kind='stable').astype(np.int32))


def rows_ref(cs, start, roff, score, key):
    hoff, site, _, s = H.entries_ref(cs, start, roff, score, key)
    return rows_from_entries(hoff, site, s, len(key))


# ---------------------------------------------------------------------------------------------------------------- (a) the device's order

def term(s, th):
    t = -math.expm1(-abs(s))
    return math.log1p(-((1.0 - th if s >= 0.0 else th) * t))


def post(s, th):
    t = -math.expm1(-abs(s))
    return th / (1.0 - (1.0 - th) * t) if s >= 0.0 else th * (1.0 - t) / (1.0 - th * t)


def _group16_sum(v):
    """the first four steps of the library's wave sum on one row of 16 lanes: lane 0's word"""
    l = np.arange(16)
    v = v + v[l ^ 1]
    v = v + v[l ^ 2]
    v = v + v[(l & ~7) | (7 - (l & 7))]
    v = v + v[15 - l]
    return v[0]


def threads_sum(per):
    """the words of 16, 64 or 256 threads summed as the device does"""
    if len(per) == 16:
        return float(_group16_sum(per))
    tot = np.float64(0.0)
    if len(per) == 64:
        return float(H._wave_sum(per))
    for w in range(len(per) // 64):
        tot = tot + H._wave_sum(per[64 * w:64 * w + 64])
    return float(tot)


def batch_sums(hoff, ll, gamma, theta_in=None, theta_out=None, n_site=None):
    """`sums` from per-read values in the fixed order: thread t adds reads t, t + 256, ... with an entry"""
    n = len(hoff) - 1
    gamma = np.asarray(gamma, np.float64).reshape(n, -1)
    nc = gamma.shape[1]
    m = np.diff(hoff)
    steps = -(-n // 256)
    words = np.zeros((3 + nc, steps * 256))
    words[0, :n], words[1, :n], words[2, :n], words[3:, :n] = ll, 1.0, m, gamma.T
    live = np.zeros(steps * 256, bool)
    live[:n] = m > 0
    per = np.zeros((3 + nc, 256))
    for k in range(steps):                           # all 256 chains at once, a read per pass; a read without an entry adds nothing
        sl = slice(k * 256, (k + 1) * 256)
        per = np.where(live[sl][None, :], per + words[:, sl], per)
    out = np.zeros(SUMS + nc)
    out[0], out[1], out[2] = (threads_sum(per[i]) for i in range(3))
    if theta_in is not None:
        cells = np.asarray(n_site).reshape(-1) > 0.0
        move = np.abs(np.asarray(theta_out).reshape(-1) - np.asarray(theta_in).reshape(-1))[cells]
        out[3] = move.max() if len(move) else 0.0
    for c in range(nc):
        out[SUMS + c] = threads_sum(per[3 + c])
    return out


def site_ref(s_rows, gamma_rows, theta_j):
    """One site's N and Mo [C] in the device's order, from the scores of its rows (in the order of its list), the gamma [n, C] of their
    reads and theta_in[j]: thread g adds rows g, g + G, ... (all threads at once here, a step of the chains per pass), then the
    reduction of the G words"""
    s_rows, gamma_rows, theta_j = np.asarray(s_rows, np.float64), np.asarray(gamma_rows, np.float64), np.asarray(theta_j, np.float64)
    n, nc = gamma_rows.shape
    G = site_threads(n)
    steps = -(-n // G) if n else 0
    N, Mo = np.zeros(nc), np.zeros(nc)
    for c in range(nc):
        p = np.array([post(float(v), float(theta_j[c])) for v in s_rows])
        gm = np.zeros(steps * G)
        gp = np.zeros(steps * G)
        gm[:n], gp[:n] = gamma_rows[:, c], gamma_rows[:, c] * p
        live = (np.arange(steps * G) < n).reshape(steps, G)
        pn, pm = np.zeros(G), np.zeros(G)
        for k in range(steps):                       # (a thread beyond the rows adds nothing: 0.0 + x is x, and -0.0 does not occur)
            pn = np.where(live[k], pn + gm[k * G:(k + 1) * G], pn)
            pm = np.where(live[k], pm + gp[k * G:(k + 1) * G], pm)
        N[c], Mo[c] = threads_sum(pn), threads_sum(pm)
    return N, Mo


def step_ref(rows, theta, w):
    """One EM step, sequential float64 in the header's ORDER -> dict(gamma [nreads, C], ll, cls, status, theta_out, n_site [nsites, C],
    w_out, sums)"""
    hoff, site, s, rread, soff, srow = (rows[f] for f in ('hoff', 'site', 's', 'rread', 'soff', 'srow'))
    theta = np.asarray(theta, np.float64)
    nsites, nc = theta.shape
    n = len(hoff) - 1
    gamma, ll = np.zeros((n, nc)), np.zeros(n)
    cls, status = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    logw = [math.log(float(v)) for v in w]
    for r in range(n):
        base, m = int(hoff[r]), int(hoff[r + 1] - hoff[r])
        if m == 0:
            status[r] = NO_SITE
            continue
        T = read_threads(m)
        per = np.zeros((nc + 1, T))
        for k in range(m):
            t, sc = k % T, float(s[base + k])
            th = theta[site[base + k]]
            for c in range(nc):
                per[c, t] += term(sc, float(th[c]))
            per[nc, t] += max(sc, 0.0)
        a = [logw[c] + threads_sum(per[c]) for c in range(nc)]
        S = threads_sum(per[nc])
        M = a[0]
        for c in range(1, nc):
            if a[c] > M:
                M = a[c]
        x = [math.exp(v - M) for v in a]
        Z = 0.0
        for v in x:
            Z += v
        best = 0
        for c in range(nc):
            gamma[r, c] = x[c] / Z
            if gamma[r, c] > gamma[r, best]:
                best = c
        ll[r] = (M + math.log(Z)) + S
        cls[r] = best
    theta_out, n_site = theta.copy(), np.zeros((nsites, nc))
    for j in range(nsites):
        lst = srow[soff[j]:soff[j + 1]]
        if len(lst) == 0:
            continue
        N, Mo = site_ref(s[lst], gamma[rread[lst]], theta[j])
        n_site[j] = N
        for c in range(nc):
            if N[c] > 0.0:
                theta_out[j, c] = min(max(Mo[c] / N[c], LO), HI)
    sums = batch_sums(hoff, ll, gamma, theta, theta_out, n_site)
    w_out = sums[SUMS:] / sums[1] if sums[1] > 0.0 else np.asarray(w, np.float64).copy()
    return dict(gamma=gamma, ll=ll, cls=cls, status=status, theta_out=theta_out, n_site=n_site, w_out=w_out, sums=sums)


# ---------------------------------------------------------------------------------------------------------------- (b) mpmath and the gates

def step_mp(rows, theta, w, dps=50):
    """The same step in mpmath at `dps` digits, theta, w and s taken as the exact doubles they are, 1 - th as the double the device
    forms.  Returns dict: gamma (list of lists), ll, theta_out, n_site (lists, mpf); status; margin (float[nreads], the two largest
    gamma apart; 1 with one class); and the gates as float arrays: g_ll, scale_ll (D), g_gamma [nreads]; g_theta, g_n [nsites, C]"""
    import mpmath as mp
    hoff, site, s, rread, soff, srow = (rows[f] for f in ('hoff', 'site', 's', 'rread', 'soff', 'srow'))
    theta = np.asarray(theta, np.float64)
    nsites, nc = theta.shape
    n, nrows = len(hoff) - 1, len(s)
    with mp.workdps(dps):
        one = mp.mpf(1)
        th_mp = [[mp.mpf(float(v)) for v in row] for row in theta]
        q_mp = [[mp.mpf(1.0 - float(v)) for v in row] for row in theta]       # the double 1 - th
        t_mp = [-mp.expm1(-abs(mp.mpf(float(v)))) for v in s]
        logw = [mp.log(mp.mpf(float(v))) for v in w]
        gamma, ll = [[mp.mpf(0)] * nc for _ in range(n)], [mp.mpf(0)] * n
        status = np.zeros(n, np.uint8)
        g_ll, scale_ll, g_gamma, margin = np.zeros(n), np.ones(n), np.zeros(n), np.ones(n)
        post_mp = [None] * nrows
        g_post = np.zeros((nrows, nc))
        for r in range(n):
            base, m = int(hoff[r]), int(hoff[r + 1] - hoff[r])
            if m == 0:
                status[r] = NO_SITE
                continue
            l = [mp.mpf(0)] * nc
            amp, absg, S = np.zeros(nc), np.zeros(nc), mp.mpf(0)
            for k in range(m):
                row = base + k
                j, up, t = int(site[row]), s[row] >= 0.0, t_mp[row]
                S += max(mp.mpf(float(s[row])), 0)
                ps = []
                for c in range(nc):
                    th = th_mp[j][c]
                    x = (q_mp[j][c] if up else th) * t
                    d = one - x
                    g = mp.log(d)
                    l[c] += g
                    xd = float(x) / float(d)
                    amp[c] += xd; absg[c] -= float(g)
                    p = th / d if up else th * (one - t) / d
                    ps.append(p)
                    g_post[row, c] = U * ((0.0 if up else (EXP_U + 2) * float(theta[j, c]) / float(d)) + float(p) * (X_U * xd + 2))
                post_mp[row] = ps
            su = sum_u(m, read_threads(m))
            a = [logw[c] + l[c] for c in range(nc)]
            g_a = [U * (X_U * amp[c] + (EXP_U + su + 1) * absg[c] + (EXP_U + 2) * float(abs(logw[c]))) for c in range(nc)]
            M = max(a)
            x = [mp.exp(v - M) for v in a]
            Z = mp.fsum(x)
            gamma[r] = [v / Z for v in x]
            ll[r] = M + mp.log(Z) + S
            top = sorted((float(v) for v in gamma[r]), reverse=True)
            margin[r] = top[0] - top[1] if nc > 1 else 1.0
            g_gamma[r] = 4 * max(g_a) + (2 * EXP_U + nc + 2) * U
            g_ll[r] = 3 * max(g_a) + U * ((su + 3) * (float(S) + max(float(abs(v)) for v in a)) + 2 * EXP_U + nc + 4)
            scale_ll[r] = absg.max() + float(S) + 1.0
        theta_out = [[None] * nc for _ in range(nsites)]
        n_site = [[None] * nc for _ in range(nsites)]
        g_theta, g_n = np.zeros((nsites, nc)), np.zeros((nsites, nc))
        for j in range(nsites):
            lst = srow[soff[j]:soff[j + 1]]
            su = sum_u(len(lst), site_threads(len(lst)))
            for c in range(nc):
                N = Mo = mp.mpf(0)
                e_n = e_mo = 0.0
                for row in lst:
                    gm, p = gamma[rread[row]][c], post_mp[row][c]
                    N += gm; Mo += gm * p
                    e_n += g_gamma[rread[row]]
                    e_mo += float(gm) * g_post[row, c] + float(p) * g_gamma[rread[row]] + U * float(gm * p)
                th = min(max(Mo / N, mp.mpf(LO)), mp.mpf(HI)) if N > 0 else th_mp[j][c]
                theta_out[j][c], n_site[j][c] = th, N
                g_n[j, c] = e_n + su * U * float(N)
                g_theta[j, c] = (e_mo + su * U * float(Mo)) + float(th) * g_n[j, c] + U * float(th * N)
    return dict(gamma=gamma, ll=ll, status=status, margin=margin, theta_out=theta_out, n_site=n_site, g_ll=g_ll, scale_ll=scale_ll,
                g_gamma=g_gamma, g_theta=g_theta, g_n=g_n)


def errors_against_mp(res, exact):
    """The errors of a step's float outputs (dict of numpy arrays, gamma / theta_out / n_site of any shape) against step_mp's, each in
    units of its gate: dict(ll, gamma, theta_out, n_site) of float arrays; <= 1 passes.  A gate of 0 (no entry, no row) asks for 0."""
    import mpmath as mp
    n, nc = len(exact['ll']), len(exact['gamma'][0]) if exact['gamma'] else 0
    gamma = np.asarray(res['gamma'], np.float64).reshape(n, -1) if 'gamma' in res else None
    out = {}
    with mp.workdps(50):
        def units(err, gate):
            err = float(err)
            return 0.0 if err == 0.0 else (math.inf if gate == 0.0 else err / gate)
        if 'll' in res:
            out['ll'] = np.array([units(abs(mp.mpf(float(res['ll'][r])) - exact['ll'][r]), exact['g_ll'][r]) for r in range(n)])
        if gamma is not None:
            out['gamma'] = np.array([[units(abs(mp.mpf(float(gamma[r, c])) - exact['gamma'][r][c]), exact['g_gamma'][r]) for c in range(nc)]
                                     for r in range(n)]).reshape(n, nc)
        ns = len(exact['theta_out'])
        if 'theta_out' in res:
            th = np.asarray(res['theta_out'], np.float64).reshape(ns, -1)
            out['theta_out'] = np.array([[units(abs(mp.mpf(float(th[j, c])) - exact['theta_out'][j][c]) * exact['n_site'][j][c], exact['g_theta'][j, c])
                                          for c in range(nc)] for j in range(ns)]).reshape(ns, nc)
        if 'n_site' in res:
            ng = np.asarray(res['n_site'], np.float64).reshape(ns, -1)
            out['n_site'] = np.array([[units(abs(mp.mpf(float(ng[j, c])) - exact['n_site'][j][c]), exact['g_n'][j, c]) for c in range(nc)]
                                      for j in range(ns)]).reshape(ns, nc)
    return out


def decided(exact):
    """the reads whose class the gate decides: an entry, and the two largest gamma further apart than 2 G_GAMMA"""
    return (exact['status'] == 0) & (exact['margin'] > 2.0 * exact['g_gamma'])


# ---------------------------------------------------------------------------------------------------------------- vectorised and dense

def _finish(hoff, l, S, w, theta, site, s, rread, post_rows):
    n, nc = l.shape
    has = np.diff(hoff) > 0
    a = np.log(np.asarray(w, np.float64))[None, :] + l
    M = a.max(1)
    x = np.exp(a - M[:, None])
    Z = x.sum(1)
    gamma = np.where(has[:, None], x / Z[:, None], 0.0)
    ll = np.where(has, M + np.log(Z) + S, 0.0)
    cls = np.where(has, gamma.argmax(1), -1).astype(np.int32)
    N, Mo = np.zeros_like(theta), np.zeros_like(theta)
    np.add.at(N, site, gamma[rread])
    np.add.at(Mo, site, gamma[rread] * post_rows)
    with np.errstate(invalid='ignore', divide='ignore'):
        theta_out = np.where(N > 0.0, np.clip(Mo / N, LO, HI), theta)
    r1 = float(has.sum())
    cells = N > 0.0
    sums = np.concatenate(([ll.sum(), r1, float(np.diff(hoff).sum()), np.abs(theta_out - theta)[cells].max() if cells.any() else 0.0], gamma.sum(0)))
    w_out = gamma.sum(0) / r1 if r1 > 0 else np.asarray(w, np.float64).copy()
    return dict(gamma=gamma, ll=ll, cls=cls, status=np.where(has, 0, NO_SITE).astype(np.uint8), theta_out=theta_out, n_site=N, w_out=w_out, sums=sums)


def step_vec(rows, theta, w):
    """the step vectorised over the rows (numpy's order of additions): what em_ref runs on"""
    hoff, site, s, rread = (rows[f] for f in ('hoff', 'site', 's', 'rread'))
    theta = np.asarray(theta, np.float64)
    n = len(hoff) - 1
    t = -np.expm1(-np.abs(s))[:, None]
    up = (s >= 0.0)[:, None]
    th = theta[site]
    g = np.log1p(-(np.where(up, 1.0 - th, th) * t))
    l = np.zeros((n, theta.shape[1]))
    np.add.at(l, rread, g)
    S = np.bincount(rread, weights=np.maximum(s, 0.0), minlength=n)
    with np.errstate(invalid='ignore', divide='ignore'):
        p = np.where(up, th / (1.0 - (1.0 - th) * t), th * (1.0 - t) / (1.0 - th * t))
    return _finish(hoff, l, S, w, theta, site, s, rread, p)


def step_dense(rows, theta, w):
    """Brute force: every read x site x class of a dense [nreads, nsites] score matrix with a mask of the entries; the model written
    with K19's scaled emissions, log((1 - th) e_0 + th e_1), not with log1p -> dict(gamma, ll, cls, theta_out, n_site, w_out)"""
    hoff, site, s, rread = (rows[f] for f in ('hoff', 'site', 's', 'rread'))
    theta = np.asarray(theta, np.float64)
    nsites, nc = theta.shape
    n = len(hoff) - 1
    dense, mask = np.zeros((n, nsites)), np.zeros((n, nsites), bool)
    dense[rread, site] = s
    mask[rread, site] = True
    e = np.exp(-np.abs(dense))
    e0, e1 = np.where(dense > 0.0, e, 1.0), np.where(dense < 0.0, e, 1.0)
    lik = (1.0 - theta)[None] * e0[:, :, None] + theta[None] * e1[:, :, None]                      # [n, nsites, C]
    l = np.where(mask[:, :, None], np.log(lik), 0.0).sum(1)
    S = np.where(mask, np.maximum(dense, 0.0), 0.0).sum(1)
    has = mask.any(1)
    a = np.log(np.asarray(w, np.float64))[None] + l
    M = a.max(1, keepdims=True)
    x = np.exp(a - M)
    gamma = np.where(has[:, None], x / x.sum(1, keepdims=True), 0.0)
    ll = np.where(has, M[:, 0] + np.log(x.sum(1)) + S, 0.0)
    p = theta[None] * e1[:, :, None] / lik
    N = np.where(mask[:, :, None], gamma[:, None, :], 0.0).sum(0)
    Mo = np.where(mask[:, :, None], gamma[:, None, :] * p, 0.0).sum(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        theta_out = np.where(N > 0.0, np.clip(Mo / N, LO, HI), theta)
    r1 = has.sum()
    return dict(gamma=gamma, ll=ll, cls=np.where(has, gamma.argmax(1), -1), theta_out=theta_out, n_site=N,
                w_out=gamma.sum(0) / r1 if r1 else np.asarray(w, np.float64).copy())


# ---------------------------------------------------------------------------------------------------------------- (c) the loop

def em_ref(rows, theta0, w0, tol=1e-9, max_iter=500, step=step_vec):
    """EM from (theta0, w0): a step at the current parameters gives SUM ll there and the next parameters; the loop stops when SUM ll
    rose by at most tol (|ll| + 1) since the step before, or after max_iter steps -> dict(theta, w, ll, trace, n_iter, converged, last:
    the last step's outputs, at (theta, w))"""
    theta, w = np.asarray(theta0, np.float64), np.asarray(w0, np.float64)
    trace, prev, converged, res = [], None, False, None
    for _ in range(max_iter):
        res = step(rows, theta, w)
        ll = float(res['sums'][0])
        trace.append(ll)
        if prev is not None and ll - prev <= tol * (abs(ll) + 1.0):
            converged = True
            break
        if len(trace) == max_iter:
            break
        prev, theta, w = ll, res['theta_out'], res['w_out']
    return dict(theta=theta, w=w, ll=trace[-1], trace=trace, n_iter=len(trace), converged=converged, last=res)


# ---------------------------------------------------------------------------------------------------------------- the planted sample

def planted_rows(seed=220, n_reads=600, n_sites=40, coverage=0.6, shares=(0.35, 0.65), d=2.0, high=0.8, low=0.1):
    """Two planted classes of reads: class 0 (share shares[0]) has theta `high` on the first half of the sites and `low` on the second,
    class 1 the reverse.  A read covers a site with probability `coverage`; its score there is the log-likelihood ratio of N(d, 1)
    against N(0, 1) at a draw from the state's law, d (x - d / 2).  Returns (rows, z: the planted class per read, theta: [n_sites, 2])"""
    rng = np.random.default_rng(seed)
    z = (rng.random(n_reads) >= shares[0]).astype(np.int64)
    theta = np.empty((n_sites, 2))
    theta[:n_sites // 2, 0], theta[n_sites // 2:, 0] = high, low
    theta[:, 1] = theta[::-1, 0]
    cover = rng.random((n_reads, n_sites)) < coverage
    mod = rng.random((n_reads, n_sites)) < theta[:, z].T
    x = rng.normal(size=(n_reads, n_sites)) + d * mod
    score = d * (x - d / 2.0)
    hoff = np.zeros(n_reads + 1, np.int64)
    hoff[1:] = np.cumsum(cover.sum(1))
    rr, ss = np.nonzero(cover)
    return rows_from_entries(hoff, ss, score[rr, ss], n_sites), z, theta


def planted_reads(seed=227, n_reads=240, genome_len=640, spacing=12, shares=(0.35, 0.65), shift=1.5, high=0.8, low=0.1, both_strands=False):
    """The planted classes as a read-level sample for the chain K13 -> K22, in hmm_ref.chain_inputs' manner: reads of 200 .. 300 events
    from a 3-mer model (center 0) over one short reference; the candidate sites are every `spacing`-th base on both strands; the
    modified table lies `shift` spreads higher at every k-mer.  The reads lie on '+' (with both_strands every second one on '-': the
    reads of a strand share no site with those of the other, and "the class is the strand" is then a local maximum that most starts
    of EM end in).  A read of class 0 is modified at a site of the first half
    of the reference with probability `high` and of the second half with `low`, a read of class 1 the reverse; at a modified site the
    events whose k-mer holds the site's base have the modified level.
    (reads, model, alt_model, sites: (chrom, strand, pos) arrays, z: the planted class per read)"""
    import readllr_ref as RF
    import rescale_ref as R
    k, center = 3, 0
    mean, sd = R.make_model(k, holes=False)
    mean1 = mean + shift * sd
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b'ACGT', np.uint8), genome_len)
    site_pos = np.arange(spacing, genome_len - spacing, spacing)
    lo, hi = RF.kmer_window(k, center)
    z = (rng.random(n_reads) >= shares[0]).astype(np.int64)
    chrom, strand, start, vals, bases = [], [], [], [], []
    for r in range(n_reads):
        minus = both_strands and r % 2 == 1
        n = int(rng.integers(200, 301))
        s0 = int(rng.integers(0, genome_len - n + 1))
        pos = s0 + np.arange(n) if not minus else s0 + n - 1 - np.arange(n)
        b = genome[pos] if not minus else R._COMP[genome[pos]]
        codes = R.read_codes(b, k, center)
        level = mean[codes].copy()
        for a in np.flatnonzero((site_pos >= s0 + 4) & (site_pos <= s0 + n - 5)):
            first_half = site_pos[a] < genome_len // 2
            if rng.random() < (high if first_half == (z[r] == 0) else low):
                j = int(np.flatnonzero(pos == site_pos[a])[0])
                cover = np.arange(j - lo, j + hi + 1)
                level[cover] = mean1[codes[cover]]
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
            sites, z)


def agreement(cls, z, nc=2):
    """the share of the reads with an entry (cls >= 0) whose class agrees with the planted one, up to relabelling"""
    import itertools
    has = cls >= 0
    return max(float((np.asarray(perm)[cls[has]] == z[has]).mean()) for perm in itertools.permutations(range(nc)))
