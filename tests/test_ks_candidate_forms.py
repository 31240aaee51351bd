"""The bin evaluation of the KS kernels, as formulas: the simplified general form of ks_rank.hpp / rank_hist.hpp
(maximum over the masked (cumU(k), k), minimum over the unmasked (cumL(k-1), k) with k*q clamped at m*q) and the set
of candidates its float-form pass evaluates, against a brute force over the pooled points.  CPU only."""
import numpy as np

import ks_model as M

CAPACITIES = ((8, 2, 4), (16, 4, 4), (32, 8, 4))      # (C, R, LG): lanes own R consecutive bins, as in the kernels
N_PER_CAPACITY = 7000


def test_simplified_forms_match_brute_force():
    rng = np.random.default_rng(20240607)
    n = tied_runs = full = multi = 0
    for C, R, LG in CAPACITIES:
        for _ in range(N_PER_CAPACITY):
            m = int(rng.integers(1, C + 1))                      # m = C included: no +inf pad below the sentinel
            q = int(rng.integers(m, 3 * C + 1))
            g = int(rng.integers(2, 41))                         # values on a grid of 2 .. 40: three-way ties are the rule
            S = rng.integers(0, g, m).astype(np.float32)
            Q = rng.integers(0, g, q).astype(np.float32)
            got = M.evaluate(S, Q, R, LG)
            best, att, d = M.brute_force(S, Q)
            assert got['best'] == best, (C, m, q, S, Q)
            assert {(c, k) for c, k, _, _ in got['cands']} == att, (C, m, q, S, Q)
            assert len(got['cands']) == len(att), ('a candidate handed over twice', C, m, q, S, Q)
            assert got['d'] == d, (C, m, q, S, Q)
            n += 1
            tied_runs += M.has_tied_run(S, Q)
            full += m == C
            multi += len(got['cands']) > 1
    print(n, tied_runs, full, multi)
    # the sample is not vacuous
    assert n >= 20000
    assert tied_runs >= 1000, tied_runs
    assert full >= 1000, full
    assert multi >= 200, multi


def test_unmasked_cand_b_inside_a_run_is_never_the_minimum():
    """the step of the derivation that lets cand_b go unmasked: along a run of S it falls by q per key"""
    S = np.array([1, 1, 1, 1, 5, 5, 9], dtype=np.float32)
    Q = np.array([0, 1, 1, 3, 5, 7, 9, 9, 9, 10], dtype=np.float32)
    keys, cnt, eq = M.bins(S, Q, 8)
    m, q = len(S), len(Q)
    cumL = np.cumsum(cnt)
    k = np.arange(1, 9)
    cand_b = cumL[k - 1] * m - k * q
    run_end = keys[k - 1] != keys[k]
    assert list(run_end[:7]) == [False, False, False, True, False, True, True]
    for i in range(6):
        if not run_end[i]:
            assert cand_b[i + 1] == cand_b[i] - q
    assert M.evaluate(S, Q, 2, 4)['best'] == M.brute_force(S, Q)[0] == 25


def test_cand_a_inside_a_tied_run_needs_its_mask():
    """samples of Q on a run of S: cumU(k) inside the run already counts them, and the unmasked candidate is above
    every valid one"""
    S = np.array([1, 1, 1, 1], dtype=np.float32)
    Q = np.array([1] * 9 + [2], dtype=np.float32)
    keys, cnt, eq = M.bins(S, Q, 8)
    m, q = len(S), len(Q)
    cumL = np.cumsum(cnt)
    k = np.arange(1, 9)
    cand_a = (cumL[k] - eq[k]) * m - k * q
    assert cand_a[0] == 26 and keys[0] == keys[1]
    assert M.brute_force(S, Q)[0] == 4
    assert M.evaluate(S, Q, 2, 4)['best'] == 4
