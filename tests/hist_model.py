"""numpy model of what a position does to the all-tests sorting forms of K1 (nanomod_amd/csrc/rank_hist.hpp, rank_all.hpp):
which instance takes it, which group is sorted (S) and which is ranked and scattered (Q), the bin counts the scatter and the
odd-even clean-up see, whether a sorted group sends seg_tie_pp down its general path, which runs of equal keys straddle a lane
boundary of the blocked layout and at which register offsets, and the pad counts.  test_hist_model.py (CPU) uses it to prove
that every constructed position of hist_cases.py has the property it is named for.

Blocked layout: element i of a sorted group sits in register i % R of lane i // R of the position's LG lanes; C = R * LG."""
import numpy as np


def size_class_of(n):
    """rank_stats_launch.hpp: the smallest class c with 64 << c >= n (6: beyond the wave-resident kernels)"""
    c = 0
    while c < 6 and n > (64 << c):
        c += 1
    return c


def instance_of(n0, n1):
    """the all-tests sorting form of an n0 v n1 position (classify_position / class_forms, rank_stats_launch.hpp):
    ('rank_hist', R, LG), ('rank_pair', R0, R1), ('wide',) or ('big',)"""
    c0, c1 = size_class_of(n0), size_class_of(n1)
    cm, cl = max(c0, c1), min(c0, c1)
    if cm >= 6:
        return ('big',)
    if cm <= 4 and cl >= cm - 1:
        lg = 8 if cm <= 1 else 16 if cm == 2 else 32 if cm == 3 else 64
        return ('rank_hist', (64 << cm) // lg, lg)
    if cl <= 2:
        return ('wide',)
    return ('rank_pair', 1 << c0, 1 << c1)


def split(a, b):
    """-> (S, Q, swap): S is the smaller group, group 1 when the sizes are equal (rank_hist.hpp: d.swap = n1 < n0)"""
    swap = len(b) < len(a)
    return (b, a, True) if swap else (a, b, False)


def has_triple(x):
    """a key of the sorted group equals both of its predecessors: seg_tie_pp leaves its fast path"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    return bool(len(x) >= 3 and np.any((x[2:] == x[1:-1]) & (x[1:-1] == x[:-2])))


def runs_of(x):
    """[(start, end, value)] of the runs of equal keys of the sorted group (end exclusive)"""
    x = np.sort(np.asarray(x, dtype=np.float64))
    if len(x) == 0:
        return []
    cut = np.flatnonzero(np.r_[True, x[1:] != x[:-1], True])
    return [(int(s), int(e), float(x[s])) for s, e in zip(cut[:-1], cut[1:])]


def straddles(x, R):
    """the runs of two or more equal keys that cross a lane boundary: [(lane boundary index i = R * j, the run's register offsets
    in the lane below, ... in the lane above)], e.g. (R * j, (R - 1,), (0,)) for a pair at (R - 1 | 0)"""
    out = []
    for s, e, _ in runs_of(x):
        if e - s < 2:
            continue
        for bnd in range((s // R + 1) * R, e, R):
            left = tuple(i % R for i in range(max(s, bnd - R), bnd))
            right = tuple(i % R for i in range(bnd, min(e, bnd + R)))
            out.append((bnd, left, right))
    return out


def describe(a, b, R, LG):
    """What rank_hist_kernel<R, LG> sees of the position (a, b).  Returns a dict:
    m, q, swap        sizes of S and Q, whether group 2 is S
    cntL              [C + 1] bin counts #{x in Q : #{s < x} = j}; maxc their maximum: the odd-even phases this position asks of
                      its whole wave
    eq                [C + 1] samples of Q equal to key j of S, counted at the first key of the run
    ab1, ab3          sum over the runs of S tied with Q of a b and a b (a + b)
    general_s/_q      seg_tie_pp's general path for sorted S / sorted Q
    straddle_s/_q     straddles() of sorted S / sorted Q
    pad_s, pad_q      +inf pads behind S / words past q in Q's read-back"""
    C = R * LG
    S, Q, swap = split(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    S = np.sort(S); m, q = len(S), len(Q)
    assert 1 <= m <= q <= C
    keys = np.full(C + 1, np.inf); keys[:m] = S
    L = np.searchsorted(S, Q, side='left')
    cntL = np.bincount(L, minlength=C + 1).astype(np.int64)
    eq = np.bincount(L, weights=(keys[L] == Q), minlength=C + 1).astype(np.int64)
    ab1 = ab3 = 0
    for s, e, _ in runs_of(S):
        ab1 += (e - s) * int(eq[s]); ab3 += (e - s) * int(eq[s]) * (e - s + int(eq[s]))
    return {'m': m, 'q': q, 'swap': swap, 'cntL': cntL, 'maxc': int(cntL.max()), 'eq': eq, 'ab1': ab1, 'ab3': ab3,
            'general_s': has_triple(S), 'general_q': has_triple(Q), 'straddle_s': straddles(S, R), 'straddle_q': straddles(Q, R),
            'pad_s': C - m, 'pad_q': C - q}


def describe_pair(a, b, R0, R1):
    """What rank_pair_kernel<R0, R1> sees: the pads behind each sorted group (their run of +inf adds pad_run_pp to the tie sum and
    is subtracted again) and which group is ranked into the other (the one with fewer samples; group 2 when equal)"""
    n0, n1 = len(a), len(b)
    assert 1 <= n0 <= 64 * R0 and 1 <= n1 <= 64 * R1
    return {'pad0': 64 * R0 - n0, 'pad1': 64 * R1 - n1, 'ranked': 1 if n1 <= n0 else 0}


def pad_run_pp(P):
    """sum_{p = 1..P} p (p - 1): what a run of P pads adds"""
    return (P - 1) * P * (P + 1) // 3


def count_window_tails(a, b):
    """int16 keys: how many samples of the position the counting forms' probe (cnt_wide_probe_kernel, rank_count_wide.hpp) finds
    outside the 2 048-value window it expects the kernel to pick — around the mean of S (the smaller group; group 1 when equal),
    then around the mean of S's samples within 1 024 of that.  The probe lets a position in with at most 32 of them (96 where both
    groups exceed 1 024 samples) and opens a class to the counting form when 7 of 8 sampled positions are let in and, below that
    size, the tail samples are at most 20 per mille of theirs."""
    a = np.asarray(a, dtype=np.int64); b = np.asarray(b, dtype=np.int64)
    S = b if len(b) < len(a) else a
    c0 = int(np.rint(np.float32(S.sum()) / np.float32(len(S))))
    d = S - c0
    near = d[(d >= -1024) & (d < 1024)]
    c = c0 + int(np.rint(np.float32(near.sum()) / np.float32(len(near)))) if len(near) else c0
    base = max(-32768, min(c - 1024, 32768 - 2048))
    return int(sum(np.count_nonzero((x < base) | (x >= base + 2048)) for x in (a, b)))
