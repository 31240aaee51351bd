"""numpy model of the KS kernels' bin evaluation (nanomod_amd/csrc/ks_rank.hpp, general form) and of the candidates
its float-form pass evaluates, next to a brute force over the pooled points.  Shared by test_ks_candidate_forms.py
(CPU) and test_ks_eval_gpu.py (which uses it to prove what its constructed positions exercise).

S is the smaller group (m samples), Q the other (q samples); the sorted S is padded with +inf to the capacity
C = R * LG (key C is the +inf sentinel).  Lane l of the LG lanes of a position owns the bins k = l*R + 1 .. l*R + R."""
import numpy as np


def bins(S, Q, C):
    """keys[0..C] (sorted S, +inf pads), cnt[L] = #{x : L(x) = L}, eq[L] = #{x : L(x) = L and x == keys[L]}, L(x) = #{s < x}"""
    S = np.sort(np.asarray(S, dtype=np.float64))
    Q = np.asarray(Q, dtype=np.float64)
    m = S.shape[0]
    assert 1 <= m <= C
    keys = np.full(C + 1, np.inf)
    keys[:m] = S
    L = np.searchsorted(S, Q, side='left')
    e = keys[L] == Q
    cnt = np.bincount(L, minlength=C + 1).astype(np.int64)
    eq = np.bincount(L, weights=e, minlength=C + 1).astype(np.int64)
    return keys, cnt, eq


def evaluate(S, Q, R, LG):
    """The simplified formulas.  Returns a dict:
    best      the integer maximum max |c*m - k*q|
    hits      the lanes whose own maximum equals best (the trips of the float-form pass), none when best == 0
    cands     the (c, k, lane, kind) handed to the float form: kind 'b' = (cumL(k-1), k), 'a' = (cumU(k), k), '0' = (cumU(0), 0)
    d         max over cands of |fl(k/m) - fl(c/q)| (0.0 without candidates)"""
    C = R * LG
    m, q = len(S), len(Q)
    keys, cnt, eq = bins(S, Q, C)
    cumL = np.cumsum(cnt)
    k = np.arange(1, C + 1, dtype=np.int64)
    clp = cumL[k - 1]
    cu = cumL[k] - eq[k]
    run_end = keys[k - 1] != keys[k]                      # +inf pads: holds at k = m, fails for k > m
    nkq = np.maximum(-k * q, -m * q)                      # k*q clamped at m*q: the pads' cand_b becomes 0
    cand_b = clp * m + nkq                                # no mask
    cand_a = np.where(run_end, cu * m + nkq, 0)           # masked
    cu0 = int(cnt[0] - eq[0])
    hi = cand_a.reshape(LG, R).max(axis=1)
    hi = np.maximum(hi, 0)
    hi[0] = max(hi[0], cu0 * m)
    lo = np.minimum(cand_b.reshape(LG, R).min(axis=1), 0)
    lbest = np.maximum(hi, -lo)
    best = int(lbest.max())
    cands = []
    hits = []
    if best != 0:
        hits = [int(l) for l in np.nonzero(lbest == best)[0]]
        if 0 in hits and cu0 * m == best:
            cands.append((cu0, 0, 0, '0'))
        for l in hits:
            for kk in range(l * R + 1, l * R + R + 1):
                i = kk - 1
                if not run_end[i]:
                    continue
                hb = abs(int(clp[i]) * m - kk * q) == best
                ha = abs(int(cu[i]) * m - kk * q) == best and not (hb and cu[i] == clp[i])
                if hb:
                    cands.append((int(clp[i]), kk, l, 'b'))
                if ha:
                    cands.append((int(cu[i]), kk, l, 'a'))
    d = 0.0
    for c, kk, _, _ in cands:
        d = max(d, abs(np.float64(kk) / np.float64(m) - np.float64(c) / np.float64(q)))
    return {'best': best, 'hits': hits, 'cands': cands, 'd': float(d)}


def brute_force(S, Q):
    """Over all pooled points v: (c, k) = (#{x <= v}, #{s <= v}).  Returns (max |c*m - k*q|, the set of (c, k) that
    attain it — empty when it is 0 —, max |fl(k/m) - fl(c/q)| over ALL pooled points: ks_2samp's D)"""
    S = np.sort(np.asarray(S, dtype=np.float64))
    Q = np.sort(np.asarray(Q, dtype=np.float64))
    m, q = S.shape[0], Q.shape[0]
    pooled = np.unique(np.concatenate([S, Q]))
    k = np.searchsorted(S, pooled, side='right').astype(np.int64)
    c = np.searchsorted(Q, pooled, side='right').astype(np.int64)
    num = np.abs(c * m - k * q)
    best = int(num.max())
    att = set()
    if best != 0:
        att = {(int(ci), int(ki)) for ci, ki in zip(c[num == best], k[num == best])}
    d = float(np.max(np.abs(k / np.float64(m) - c / np.float64(q))))
    return best, att, d


def has_tied_run(S, Q):
    """a run of S (two or more equal keys) that a sample of Q sits on"""
    v, n = np.unique(np.asarray(S), return_counts=True)
    return bool(np.isin(v[n >= 2], np.asarray(Q)).any())
