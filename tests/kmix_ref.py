"""The definition of nmod_kmer_mix (include/nanomod_hip.h, K17) restated in numpy, its EM in 40-digit mpmath, and the seeded inputs the
CPU tests and the GPU tests share.  Written from the header's text; the reference project has no such step.

Per k-mer code c: usable iff mean0 and sd0 are finite, sd0 > 0 and |mean0| <= 1000; the window is the integers lo .. lo + 4 095 with
lo = llrint(1000 mean0) - 2 048; a sample has the integer k (int16: the value, floats: rint(1000 x)); hist[b] counts the samples with
k == lo + b; the EM is K8's with the weights hist[b] at x_b = (lo + b) / 1000."""
import math

import numpy as np

HALF, BINS = 2048, 4096
NOT_CONVERGED, DEGENERATE, NO_MODEL, VAR_FLOORED, TOO_FEW = 1, 2, 4, 8, 16
EQUAL, FREE = 0, 1
MODEL_BY_NAME = {'equal': EQUAL, 'free': FREE}
ST_EMPTY, ST_TOO_LARGE, ST_NONFINITE, ST_NO_CODE = 4, 8, 16, 64
MAX_DEEP = 2 ** 24 - 1
FIELDS = ('pi', 'mu_mod', 'sd_mod', 'llr')
CHUNK = 256                      # kmer_mix.hip: kKmixChunk, the positions of one work item of the histogram kernel


def usable(mean0, sd0):
    mean0, sd0 = np.asarray(mean0, np.float64), np.asarray(sd0, np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(mean0) & np.isfinite(sd0) & (sd0 > 0.0) & (np.abs(mean0) <= 1000.0)


def window_lo(mean0):
    """lo per code (0 where the code is unusable: ask usable())"""
    m = np.asarray(mean0, np.float64)
    with np.errstate(invalid='ignore'):
        ok = np.abs(m) <= 1000.0
    return np.where(ok, np.rint(1000.0 * np.where(ok, m, 0.0)), 0.0).astype(np.int64) - HALF


def sample_k(sig):
    """(k as float64 — NaN where the sample is not finite —, finite mask) of a sample vector of any of the three dtypes"""
    sig = np.asarray(sig)
    if sig.dtype == np.int16:
        return sig.astype(np.float64), np.ones(len(sig), bool)
    x = sig.astype(np.float64)
    fin = np.isfinite(x)
    with np.errstate(over='ignore', invalid='ignore'):
        return np.rint(1000.0 * np.where(fin, x, np.nan)), fin


def hist(sig, off, code, ncodes, mean0, sd0):
    """the integers of the definition: hist (ncodes x BINS, uint32), n_used, n_outside, n_positions (int64), pos_status (uint8), lo"""
    off = np.asarray(off, np.int64)
    code = np.asarray(code, np.int64)
    npos = len(code)
    ok, lo = usable(mean0, sd0), window_lo(mean0)
    k, fin = sample_k(sig)
    n = np.diff(off)
    st = np.where((code < 0) | (code >= ncodes), ST_NO_CODE, 0) | np.where(n <= 0, ST_EMPTY, 0) | np.where(n > MAX_DEEP, ST_TOO_LARGE, 0)
    h = np.zeros((ncodes, BINS), np.int64)
    n_out, n_pos = np.zeros(ncodes, np.int64), np.zeros(ncodes, np.int64)
    for p in np.flatnonzero(st == 0):
        c = int(code[p])
        if not ok[c]:
            continue
        kp, fp = k[off[p]:off[p + 1]], fin[off[p]:off[p + 1]]
        if not fp.all():
            st[p] |= ST_NONFINITE
        with np.errstate(invalid='ignore'):
            inside = fp & (kp >= lo[c]) & (kp < lo[c] + BINS)
        h[c] += np.bincount((kp[inside] - lo[c]).astype(np.int64), minlength=BINS)
        n_out[c] += int((~inside).sum())
        n_pos[c] += int(inside.any())
    assert h.max(initial=0) < 2 ** 32
    return dict(hist=h.astype(np.uint32), n_used=h.sum(axis=1), n_outside=n_out, n_positions=n_pos, pos_status=st.astype(np.uint8), lo=lo,
                usable=ok)


def softplus(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _t(x, mu, s2, pi, m, v, model):
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        t = np.log((1.0 - pi) / pi)
        if model == FREE:
            t = t + 0.5 * np.log(v / s2)
        return t + (x - m) ** 2 / (2.0 * v) - (x - mu) ** 2 / (2.0 * s2)


def _nan(status):
    r = {f: np.nan for f in FIELDS}
    r.update(iters=0, status=status, delta=np.nan, delta_prev=np.nan)
    return r


def _bins(h, lo):
    """the non-empty bins: (weights as float64, x, n, S1) — an empty bin adds exactly 0.0 to every sum"""
    h = np.asarray(h).astype(np.int64)
    b = np.flatnonzero(h)
    ks = int(lo) + b
    n, s1 = int(h.sum()), int((h[b] * ks).sum())
    return h[b].astype(np.float64), ks.astype(np.float64) / 1000.0, n, s1


def _run(h, lo, mean0, sd0, model, max_iter, tol, fixed, min_samples=2):
    if not bool(usable(mean0, sd0)):
        return _nan(NO_MODEL)
    w, x, n, s1 = _bins(h, lo)
    if n < max(int(min_samples), 2):
        return _nan(TOO_FEW)
    mu, s = float(mean0), float(sd0)
    s2 = s * s
    ybar = (float(s1) / float(n)) / 1000.0
    pi, m, v = 0.5, mu + 2.0 * (ybar - mu), s2
    delta = delta_prev = np.nan
    floored, iters, converged = False, 0, False
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for k in range(1, max_iter + 1):
            r = w * (1.0 / (1.0 + np.exp(_t(x, mu, s2, pi, m, v, model))))
            W = float(np.sum(r))
            if not W > 0.0:
                return _nan(DEGENERATE)
            pn, mn, vn, fl = W / n, float(np.sum(r * x)) / W, v, False
            if model == FREE:
                vn = float(np.sum(r * (x - mn) ** 2)) / W
                fl = vn < s2 / 16.0
                vn = max(vn, s2 / 16.0)
            dl = max(abs(pn - pi), abs(mn - m) / s)
            if model == FREE:
                dl = max(dl, abs(math.sqrt(vn) - math.sqrt(v)) / s)
            delta_prev, delta = delta, dl
            pi, m, v, floored, iters = pn, mn, vn, fl, k
            if not fixed and tol > 0.0 and dl <= tol:
                converged = True
                break
        llr = 2.0 * float(np.sum(w * (np.log(1.0 - pi) + softplus(-_t(x, mu, s2, pi, m, v, model)))))
    status = (VAR_FLOORED if floored else 0) | (0 if converged or fixed else NOT_CONVERGED)
    return dict(pi=pi, mu_mod=m, sd_mod=math.sqrt(v), llr=llr, iters=iters, status=status, delta=delta, delta_prev=delta_prev)


def em(h, lo, mean0, sd0, model, iters):
    """exactly `iters` iterations on one code's histogram; also `delta` of the last iteration and `delta_prev` of the one before.
    status holds NO_MODEL / TOO_FEW (below 2) / DEGENERATE / VAR_FLOORED only: whether a run converged is the caller's rule"""
    return _run(h, lo, mean0, sd0, model, int(iters), 0.0, True)


def run(h, lo, mean0, sd0, model, max_iter=200, tol=1e-6, min_samples=2):
    """the whole definition of one code with its stopping rule: delta <= tol (tol > 0) or max_iter iterations"""
    return _run(h, lo, mean0, sd0, model, int(max_iter), float(tol), False, min_samples)


def em_mp(h, lo, mean0, sd0, model, iters, dps=40):
    """em in mpmath at `dps` digits (mean0, sd0 and the x_b are taken as the exact doubles they are): pi, mu_mod, sd_mod, llr as mpf"""
    import mpmath as mp
    w, x, n, _ = _bins(h, lo)
    ybar = (float(int((np.asarray(h).astype(np.int64) * (int(lo) + np.arange(len(h)))).sum())) / float(n)) / 1000.0
    with mp.workdps(dps):
        w = [mp.mpf(float(u)) for u in w]
        x = [mp.mpf(float(u)) for u in x]
        mu, s = mp.mpf(float(mean0)), mp.mpf(float(sd0))
        s2 = mp.mpf(float(sd0) * float(sd0))                  # s2 is the double s * s, as the definition has it
        pi, m, v = mp.mpf(0.5), mp.mpf(float(mean0) + 2.0 * (ybar - float(mean0))), s2      # (the start values are doubles too)
        a = [(u - mu) ** 2 / (2 * s2) for u in x]

        def tt():
            c = mp.log((1 - pi) / pi) + (mp.log(v / s2) / 2 if model == FREE else 0)
            hv = 1 / (2 * v)
            return [c + (u - m) ** 2 * hv - ai for u, ai in zip(x, a)]
        for _ in range(int(iters)):
            r = [wi / (1 + mp.exp(t)) for wi, t in zip(w, tt())]
            W = mp.fsum(r)
            pi, m = W / n, mp.fsum(ri * u for ri, u in zip(r, x)) / W
            if model == FREE:
                v = max(mp.fsum(ri * (u - m) ** 2 for ri, u in zip(r, x)) / W, s2 / 16)
        llr = 2 * mp.fsum(wi * (mp.log(1 - pi) + mp.log(1 + mp.exp(-t))) for wi, t in zip(w, tt()))
        return dict(pi=pi, mu_mod=m, sd_mod=mp.sqrt(v), llr=llr, s=s)


# ---------------------------------------------------------------------------------------------------- shared inputs
def csr(rows, dtype=np.int16):
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return (np.concatenate([np.asarray(r, dtype=dtype) for r in rows]) if rows else np.zeros(0, dtype)), off


PARITY_SHARES = (0.0, 0.1, 0.3, 0.6, 1.0)
PARITY_SIZES = (2, 3, 5, 17, 64, 200, 1000, 5000, 20000, 200000)


def parity_inputs(seed=20261020, ncodes=64):
    """The batch of the EM parity test: 64 codes with a random control table (levels in +-3, sd 0.15 .. 0.3), code c pooling
    PARITY_SIZES[c mod 10] samples in rows of at most 300, planted shares walking through PARITY_SHARES (every size meets several) at +-(3 .. 5) sd0.  int16.
    Returns (rows, code per row, mean0, sd0)."""
    rng = np.random.default_rng(seed)
    mean0 = np.round(rng.uniform(-3.0, 3.0, ncodes), 4)
    sd0 = np.round(rng.uniform(0.15, 0.3, ncodes), 4)
    rows, code = [], []
    for c in range(ncodes):
        n = PARITY_SIZES[c % len(PARITY_SIZES)]
        share = PARITY_SHARES[(c // 10 + c) % len(PARITY_SHARES)]
        shift = (3.0 + (c % 3)) * (1 if c % 2 else -1) * sd0[c]
        y = mean0[c] + sd0[c] * rng.standard_normal(n)
        y[rng.random(n) < share] += shift
        y = np.rint(1000.0 * y).astype(np.int16)
        for b in range(0, n, 300):
            rows.append(y[b:b + 300]); code.append(c)
    order = rng.permutation(len(rows))
    return [rows[i] for i in order], np.asarray(code, np.int32)[order], mean0, sd0


RECOVERY = dict(npos=3000, k=3, center=1, reads=60, shift=0.8, share=0.5, sd=0.2, jitter=0.05, seed=20261021)


def recovery_groups(cfg=RECOVERY):
    """The control and the sample of the recovery test as per-position containers: a random ACGT run, levels from a random 64-entry
    table with a position-to-position jitter of sd `jitter` inside a total sd of `sd`, on the int16 grid; in the sample the reads at
    positions of two chosen k-mers are modified with probability `share` and shifted by +`shift`.  Returns (control, sample, the two
    codes)."""
    rng = np.random.default_rng(cfg['seed'])
    npos, k, center, reads = cfg['npos'], cfg['k'], cfg['center'], cfg['reads']
    bases = rng.integers(0, 4, npos)
    table = np.round(rng.uniform(-2.5, 2.5, 4 ** k), 3)
    code = np.full(npos, -1, np.int64)
    for i in range(center, npos - (k - 1 - center)):
        c = 0
        for d in range(-center, k - center):
            c = c * 4 + int(bases[i + d])
        code[i] = c
    counts = np.bincount(code[code >= 0], minlength=4 ** k)
    chosen = np.argsort(-counts, kind='stable')[:2]                       # the two most frequent k-mers: ~ 47 positions x 60 reads each
    within = math.sqrt(cfg['sd'] ** 2 - cfg['jitter'] ** 2)

    def group(modify):
        level = np.where(code >= 0, table[np.maximum(code, 0)], 0.0) + cfg['jitter'] * rng.standard_normal(npos)
        x = level[:, None] + within * rng.standard_normal((npos, reads))
        if modify:
            hit = np.isin(code, chosen)[:, None] & (rng.random((npos, reads)) < cfg['share'])
            x = x + cfg['shift'] * hit
        sig = np.rint(1000.0 * x).astype(np.int16).reshape(-1)
        return dict(chrom=np.array(['chr1'] * npos), strand=np.array(['+'] * npos), pos=np.arange(npos, dtype=np.int64) + 100,
                    base=np.array(list('ACGT'))[bases], off=np.arange(npos + 1, dtype=np.int64) * reads, sig=sig)
    return group(False), group(True), np.sort(chosen).astype(np.int64)


def restated_alt(sample, code, mean0, sd0, model=FREE, max_iter=200, tol=1e-6):
    """the per-code estimates of the restatement for a per-position container whose rows carry `code` (-1: no part): a dict of arrays"""
    ncodes = len(mean0)
    hh = hist(sample['sig'], sample['off'], code, ncodes, mean0, sd0)
    res = {f: np.full(ncodes, np.nan) for f in FIELDS}
    res.update(iters=np.zeros(ncodes, np.int32), status=np.zeros(ncodes, np.uint8))
    for c in range(ncodes):
        o = run(hh['hist'][c], hh['lo'][c], mean0[c], sd0[c], model, max_iter, tol)
        for f in FIELDS + ('iters', 'status'):
            res[f][c] = o[f]
    res.update(n_used=hh['n_used'], n_outside=hh['n_outside'], n_positions=hh['n_positions'])
    return res
