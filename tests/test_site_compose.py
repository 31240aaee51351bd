"""nmod_site_compose (K26) without a GPU: the restatement by hand, the KKT conditions at its estimate, its agreement with K14's
restatement at n_alt = 1 (the gate the GPU comparison uses), a seeded null simulation of the per-state test, the conditions the shared
inputs must meet, and the argument checks of the C entry and the Python layers (before any device work)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import compose_ref as CR
import stoich_ref as SR
from nanomod_amd import _lib as L, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'site_compose.txt')
NO_SUCH_DEVICE = 99
INVALID, NO_DEVICE = -1, -5
nan, inf = float('nan'), float('inf')


def test_restatement_by_hand():
    """six reads, three states: state 3 closed (no finite score), read 1 partial (finite in state 1 only), read 2 finite in none; the four
    valid reads' weights, and one EM iteration from the uniform start"""
    S = np.array([[0.0, 1.0, nan, 2.0, -1.0, 800.0],
                  [1.0, inf, nan, -2.0, 0.5, -3.0],
                  [nan, nan, inf, -inf, nan, nan]])
    open_, valid, partial = CR.classify(S)
    assert open_.tolist() == [True, True, False] and valid.tolist() == [True, False, False, True, True, True] and partial.tolist() == [False, True, False, False, False, False]
    W, mx = CR.weights(S, open_, valid)
    assert mx.tolist() == [1.0, 2.0, 0.5, 800.0] and (W[3] == 0.0).all() and W[0, 3] == 0.0 and W[1, 3] == 1.0      # exp(-800) underflows: still valid
    assert np.allclose(W[:, 0], [math.exp(-1.0), math.exp(-1.0), 1.0, 0.0], rtol=1e-15)
    r = CR.row(S, min_valid=3, max_iter=1, tol=0.0)
    den = (W[0] + W[1] + W[2]) / 3.0
    want = np.array([(W[m] / 3.0 / den).sum() / 4.0 for m in range(3)] + [0.0])
    assert np.allclose(r['pi'], want, rtol=1e-15) and r['iters'] == 1 and r['open_mask'] == 3
    # (the last read has w_0 = w_2 = 0: without state 1 its den is 0, and that refit is DEGENERATE: NaN stat_1 and p_1, the rest stands)
    assert r['status'] == CR.NOT_CONVERGED | CR.DEGENERATE and np.isnan(r['stat_m'][0]) and r['stat_m'][1] >= 0.0
    assert r['n_valid'] == 4 and r['n_partial'] == 1 and np.isnan(r['stat_m'][2]) and np.isnan(r['p_m'][2]) and np.isnan(r['resp'][:, [1, 2]]).all()
    assert np.allclose(r['resp'][:, valid].sum(axis=0), 1.0, rtol=1e-15) and (r['resp'][3, valid] == 0.0).all()
    assert CR.row(S[:, :3])['status'] == CR.TOO_FEW and CR.row(S[2:, :])['status'] == CR.NO_STATE and CR.row(S[:, :0])['status'] == CR.NO_STATE
    zero = CR.row(np.zeros((2, 10)))                                         # all-zero scores: the uniform start is a fixed point, ll = 0
    assert zero['iters'] == 1 and np.allclose(zero['pi'], 1 / 3, rtol=1e-15) and abs(zero['ll']) < 1e-14 and zero['stat'] < 1e-13
    assert CR.p_boundary(0.0) == 1.0 and CR.p_boundary(1e5) == CR.DBL_MIN and abs(CR.p_boundary(3.841458820694124) - 0.025) < 1e-12


@pytest.mark.parametrize('n_alt', [1, 2, 3, 4])
def test_kkt_conditions_at_the_estimate(n_alt):
    """at the restatement's estimate, with W the weights: for an open state with a positive share mean_i w_im / den_i = 1 — EM's step is
    pi_m |mean - 1|, so within tol / pi_m at its stop — and <= 1 where the share went to 0; the same for canonical.  The shares sum to 1"""
    tol = 1e-12
    rng = np.random.default_rng(40 + n_alt)
    seen_zero = 0
    for case in range(12):
        n = (12, 60, 300)[case % 3]
        shares = rng.dirichlet(np.ones(n_alt + 1))
        if case % 2:
            shares[1 + case % n_alt] = 0.0                                   # an absent state: its share is often driven to the boundary
            shares /= shares.sum()
        S = CR.simulate_rows(rng, 1, n, shares, sep=(1.0, 2.5, 4.0)[case % 3])[0]
        r = CR.row(S, max_iter=CR.MAX_ITER, tol=tol, test=False)
        if r['status'] & CR.NOT_CONVERGED:                                   # (a share on its way to 0: EM is slow there; the KKT gate needs the stop)
            continue
        W, _ = CR.weights(S, np.ones(n_alt, bool), np.ones(n, bool))
        pi = r['pi']
        den = (pi[:, None] * W).sum(axis=0)
        mean = (W / den).mean(axis=1)
        assert abs(pi.sum() - 1.0) <= 1e-13
        for m in range(n_alt + 1):
            if pi[m] > 1e-9:
                assert abs(mean[m] - 1.0) <= 2.0 * tol / pi[m] + 1e-14, (case, m, pi, mean)
            else:
                assert mean[m] <= 1.0 + 1e-9, (case, m, pi, mean)
                seen_zero += 1
    assert n_alt == 1 or seen_zero >= 1


def test_agrees_with_k14_at_one_state():
    """n_alt = 1 on well-separated rows at tol = 1e-12: pi_1 within 100 tol of K14's restated pi, stat_1 within 100 tol relative of its stat,
    p_1 within the gate that follows from stat's (compose_ref.p_gate); ll and stat are the same number there.  The GPU test compares the
    two device entries at the same gates, so the rows must meet them in the restatements first"""
    s, off = CR.stoich_rows()
    a = CR.site_compose([s], off, min_valid=3, max_iter=CR.MAX_ITER, tol=CR.STOICH_TOL)
    b = SR.site_stoich(s, off, tol=CR.STOICH_TOL)
    assert not a['status'].any() and not any(r['status'] for r in b) and len(b) == 15
    worst = [0.0, 0.0, 0.0]
    for i, r in enumerate(b):
        assert 0.05 < r['pi'] < 0.95
        worst[0] = max(worst[0], abs(a['pi'][1, i] - r['pi']))
        worst[1] = max(worst[1], abs(a['stat_m'][0, i] / r['stat'] - 1.0))
        worst[2] = max(worst[2], abs(a['p_m'][0, i] / r['p_null'] - 1.0) / CR.p_gate(r['stat']))
        assert abs(a['stat'][i] - a['stat_m'][0, i]) <= 1e-12 * a['stat'][i]   # without the state everything is canonical: ll_without = 0
    print('compose_ref against stoich_ref: pi %.3g, stat %.3g relative, p %.3g of its gate' % tuple(worst))
    assert worst[0] <= CR.STOICH_GATE and worst[1] <= CR.STOICH_GATE and worst[2] <= 1.0


NULL_ROWS = 2000
NULL_LEVEL = 0.05


def test_null_simulation_of_the_per_state_test():
    """rows of 20 and of 200 reads where state 1 holds a share of 0.3 and state 2 is absent, 2 000 rows per cell, levels 2 spreads apart,
    through the restatement: the share of rows whose p_2 rejects at the 5 % level must not lie above the level plus two binomial
    standard errors of the cell (the upper gate alone: the boundary law is conservative when shares sit at 0).  Measured (also in
    profiles/site_compose.txt and the header of site_compose.hip): 4.1 % at 20 reads, 4.2 % at 200"""
    rng = np.random.default_rng(2600)
    recorded = open(PROFILE).read()
    for n in (20, 200):
        S = CR.simulate_rows(rng, NULL_ROWS, n, [0.7, 0.3, 0.0], sep=2.0)
        pi, stat, p, nc = CR.test_state_batch(S, 2, max_iter=CR.MAX_ITER, tol=1e-8)
        share = float((p <= NULL_LEVEL).mean())
        gate = NULL_LEVEL + 2.0 * math.sqrt(NULL_LEVEL * (1.0 - NULL_LEVEL) / NULL_ROWS)
        print('null cell of %d reads: %.4f rejected at %.2f (gate %.4f), %d fit(s) not converged, mean pi_1 %.3f' % (n, share, NULL_LEVEL, gate, int(nc.sum()), pi[:, 1].mean()))
        assert abs(pi[:, 1].mean() - 0.3) < 0.02 and (p > 0.0).all() and (p <= 1.0).all()
        assert share <= gate
        assert 'null n=%d rows=%d rejected=%.4f' % (n, NULL_ROWS, share) in recorded


@pytest.mark.parametrize('n_alt', [1, 2, 3, 4])
def test_shared_inputs_meet_the_conditions(n_alt):
    """the parity batch reaches every class and the row past the LDS stage, a closed state, partial reads (three states and more), every
    status bit but DEGENERATE and TOO_LARGE, a share at the boundary and |s| = 700; no fit stops within rounding of tol"""
    sc, off = CR.parity_batch(n_alt)
    lens = np.diff(off)
    assert {1, 2, 3, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, CR.stage_reads(n_alt) + 1, 0} <= set(lens.tolist())
    assert CR.stage_reads(n_alt) == L.load().nmod_site_compose_stage_reads(n_alt) and CR.stage_reads(n_alt) > CR.WAVE
    r = CR.site_compose(sc, off, **CR.PARITY_OPTS)
    assert not r['near_tol'].any()
    st = r['status']
    assert (st == CR.TOO_FEW).any() and (st == CR.NO_STATE).any() and (st == 0).any()
    assert n_alt < 4 or (st & CR.NOT_CONVERGED).any()
    est = (st & (CR.TOO_FEW | CR.NO_STATE | CR.DEGENERATE)) == 0
    full = (1 << n_alt) - 1
    assert n_alt == 1 or ((r['open_mask'] != full) & est).any()              # a closed state in a row with an estimate
    assert n_alt < 3 or (r['n_partial'][est] > 0).any()
    assert (np.nanmin(r['pi'][:, est], axis=0) < 1e-6).any() and (np.abs(np.stack(sc)) == 700.0).any()
    assert np.nanmax(np.abs(np.nansum(r['pi'][:, est], axis=0) - 1.0)) < 1e-12
    zero = len(lens) - 3
    assert lens[zero] == 40 and abs(r['ll'][zero]) < 1e-13 and r['iters'][zero] == 1


# ------------------------------------------------------------------------------------------------- the C entry's own refusals
def c_call(lib, npos=3, *, device=NO_SUCH_DEVICE, n_alt=2, total=None, score='x', score_null=None, off='x', stride=0, opts='x', out='x', max_iter=100,
           min_valid=3, tol=1e-9, memspace=None, prm=None, opts_size=None, out_size=None, dtype=7):
    n = npos if 0 <= npos < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 5
    sc = np.zeros(max(n, 1) * 5)
    pl, cnt = np.zeros(5 * max(n, 1)), np.zeros(max(n, 1), np.int32)
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    ptrs = (C.c_void_p * 4)(*[sc.ctypes.data] * 4)
    if score_null is not None:
        ptrs[score_null] = None
    o = L.make_compose_opts(max_iter, min_valid, tol)
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_compose_out(pi=pl.ctypes.data, n_valid=cnt.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:                                                          # (dtype 7: this entry does not read it)
        prm = L.make_params(device=device, memspace=L.MEM_HOST if memspace is None else memspace, dtype=dtype, stride0=stride)
    return lib.nmod_site_compose(C.byref(prm), npos, max(n, 1) * 5 if total is None else total, n_alt, C.addressof(ptrs) if score is not None else None,
                                 pick(off, offs), C.byref(o) if opts is not None else None, C.byref(r) if out is not None else None)


def refused_c_cases():
    cases = [('max_iter_0', dict(max_iter=0)), ('max_iter_2001', dict(max_iter=2001)), ('min_valid_0', dict(min_valid=0))]
    cases += [('tol_%r' % v, dict(tol=v)) for v in (-1e-9, nan, inf)]
    cases += [('n_alt_%d' % v, dict(n_alt=v)) for v in (0, -1, 5)]
    cases += [('score_null', dict(score=None)), ('score_entry_null_0', dict(score_null=0)), ('score_entry_null_1', dict(score_null=1))]
    cases += [('no_rows', dict(off=None)), ('stride_neg', dict(off=None, stride=-5)), ('stride_total', dict(off=None, stride=6))]
    cases += [('npos_neg', dict(npos=-1)), ('npos_2_31', dict(npos=2 ** 31 - 1)), ('total_neg', dict(total=-1)), ('total_short', dict(total=14))]
    cases += [('opts_null', dict(opts=None)), ('out_null', dict(out=None)), ('opts_size', dict(opts_size=32)), ('out_size', dict(out_size=88)), ('memspace_2', dict(memspace=2))]
    cases += [('off_down', dict(off=np.array([0, 5, 4, 15], np.int64))), ('off_neg', dict(off=np.array([-1, 5, 10, 15], np.int64)))]
    return cases


def test_site_compose_refuses_invalid_arguments_before_any_device_work():
    lib = L.load()
    call = lambda *a, **kw: c_call(lib, *a, **kw)
    assert call() == NO_DEVICE and call(off=None, stride=5) == NO_DEVICE and call(memspace=L.MEM_DEVICE) == NO_DEVICE
    assert all(call(n_alt=v) == NO_DEVICE for v in (1, 2, 3, 4)) and call(max_iter=2000, tol=0.0) == NO_DEVICE and call(n_alt=1, score_null=1) == NO_DEVICE
    assert call(0) == 0 and call(0, score_null=0) == 0
    for name, kw in refused_c_cases():
        kw = dict(kw)
        assert call(kw.pop('npos', 3), **kw) == INVALID, name
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert call(prm=bad) == INVALID
    assert lib.nmod_site_compose(None, 3, 15, 2, None, None, None, None) == INVALID


# --------------------------------------------------------------------------------------------- the Python layers: refusals
def _refused_host():
    s, off = np.zeros(20), np.arange(5, dtype=np.int64) * 5
    w = lambda scores=(s, s), off=off, **kw: ((list(scores), off), kw)
    cases = dict(no_scores=w(()), five=w((s,) * 5), lengths=w((s, s[:-1])), two_d=w((s.reshape(4, 5), s.reshape(4, 5))),
                 min_valid_0=w(min_valid=0), min_valid_half=w(min_valid=2.5), max_iter_0=w(max_iter=0), max_iter_2001=w(max_iter=2001),
                 tol_neg=w(tol=-1.0), tol_nan=w(tol=nan), tol_inf=w(tol=inf),
                 no_rows=w(off=None), stride_0=w(off=None, stride=0), ragged=w(off=None, stride=3), short=w((s[:-1], s[:-1])),
                 off_down=w(off=np.array([0, 6, 4, 20], np.int64)), off_empty=w(off=off[:0]))
    return [pytest.param(a, kw, id=name) for name, (a, kw) in cases.items()]


@pytest.mark.parametrize('args,kw', _refused_host())
def test_refused_before_the_library(args, kw):
    L.load()
    with pytest.raises(ValueError):
        engine.site_compose_host(*args, device=NO_SUCH_DEVICE, **kw)


def test_accepted_calls_reach_the_library():
    s, off = np.zeros(20), np.arange(5, dtype=np.int64) * 5
    with pytest.raises(L.NanomodLibraryError, match='nmod_site_compose'):
        engine.site_compose_host([s, s], off, device=NO_SUCH_DEVICE)
    res = engine.site_compose_host([s[:0]] * 3, np.zeros(1, np.int64), resp=True, device=NO_SUCH_DEVICE)      # no rows: no device
    assert res['pi'].shape == (4, 0) and res['p_m'].shape == (3, 0) and res['resp'].shape == (4, 0) and res['status'].shape == (0,)
    assert 'stat_m' not in engine.site_compose_host([s[:0]], np.zeros(1, np.int64), test=False, device=NO_SUCH_DEVICE)
