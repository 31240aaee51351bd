#!/usr/bin/env python3
"""Side measurement of nmod_site_diff (K15) on one GPU, not the headline bench: DeviceDetector.site_diff on fixed-stride pairs of rows
of simulated window sums, with and without the interval, alternated in one loop with
  (a) the route that existed before it for the test alone: three DeviceDetector.site_stoich calls — row 0, row 1 and their
      concatenation (a torch.cat per call) — from which stat = stat0 + stat1 - stat_concat;
  (b) the full definition of include/nanomod_hip.h in torch tensor operations (all sites at once, a mask for the sites that have
      stopped, one host read per evaluation to see whether any site still runs; the inner root nested in the outer one),
so that all see the same machine state.

Pairs of 30 v 30 and 100 v 100 scores (the 16-lane form), 400 v 400 (the wave form) and 2 000 v 2 000 (the workgroup form).  Each call
is timed by its own pair of HIP events after a warm-up; the figure is the median of `steps` calls (three at least), the spread their
minimum and maximum.  Reported per shape: sites/s, scores x evaluations/s (the evaluations of the iteration for pi_pool as the entry
counts them in `iters`; the other roots are not counted), both ratios, and the largest differences between the routes.  One JSON line
per run; --write FILE appends the record kept in profiles/site_diff.txt.

    python tools/bench_site_diff.py [--steps 3] [--warmup 1] [--scale 1.0] [--write FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nanomod_amd as nm

L = nm._lib
_T0 = time.time()
SHAPES = ((30, 200000), (100, 100000), (400, 20000), (2000, 4000))      # (scores per row, sites): 12, 20, 16 and 16 million scores
DBL_MIN = 2.2250738585072014e-308


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def make_rows(rows, n, seed, device, top):
    """window sums at sites where a share of 0 .. top is modified, the two levels 2 sd apart"""
    g = torch.Generator(device).manual_seed(seed)
    share = torch.rand(rows, 1, dtype=torch.float64, device=device, generator=g) * top
    z = (torch.rand(rows, n, dtype=torch.float64, device=device, generator=g) < share).to(torch.float64)
    x = torch.randn(rows, n, dtype=torch.float64, device=device, generator=g) + 2.0 * z
    return (2.0 * x - 2.0).contiguous()


def torch_diff(s0, s1, interval=True, max_iter=60, tol=1e-12, drop=L.STOICH_CI_DROP_95):
    """include/nanomod_hip.h's definition of nmod_site_diff over the rows of two matrices of valid scores, in tensor operations"""
    rows = [(-torch.expm1(-s.abs()), s >= 0) for s in (s0, s1)]
    nan = torch.full((s0.shape[0],), float('nan'), dtype=s0.dtype, device=s0.device)

    def ev_row(r, pi, want_g):
        t, plus = rows[r]
        qt = torch.where(plus, (1.0 - pi)[:, None], pi[:, None]) * t
        u = t / (1.0 - qt)
        return torch.where(plus, u, -u).sum(1), (torch.log1p(-qt).sum(1) if want_g else (u * u).sum(1))

    def joint(d):
        def ev(x, want_g):
            S0, X0 = ev_row(0, x, want_g)
            S1, X1 = ev_row(1, (x + d).clamp(0.0, 1.0), want_g)
            return S0 + S1, X0 + X1
        return ev

    def solve(ev, mode, run, a, b, ghat):
        a, b = a.clone(), b.clone()
        x = a + 0.5 * (b - a)
        active = run.clone()
        iters = torch.zeros_like(x, dtype=torch.int32)
        for k in range(1, max_iter + 1):
            if not bool(active.any()):
                break
            S, X = ev(x, mode != 0)
            if mode == 0:
                right, xn = S > 0, x + S / X
            else:
                h = 2.0 * (ghat - X)
                right, xn = (h > drop) if mode == 1 else (h <= drop), x + (h - drop) / (2.0 * S)
            na, nb = torch.where(right, x, a), torch.where(right, b, x)
            xn = torch.where((xn != x) & ~((xn > na) & (xn < nb)), na + 0.5 * (nb - na), xn)
            step = (xn - x).abs()
            a, b, x = torch.where(active, na, a), torch.where(active, nb, b), torch.where(active, xn, x)
            iters = torch.where(active, torch.full_like(iters, k), iters)
            active = active & ~((nb - na <= tol) | (step <= tol)) if tol > 0 else active
        return x, iters

    zero, one = torch.zeros_like(nan), torch.ones_like(nan)

    def mle(ev):
        S0, _ = ev(zero, False)
        S1, _ = ev(one, False)
        at0 = S0 <= 0
        at1 = ~at0 & (S1 >= 0)
        x, iters = solve(ev, 0, ~at0 & ~at1, zero, one, None)
        return torch.where(at0, zero, torch.where(at1, one, x)), iters
    pi0, _ = mle(lambda x, g: ev_row(0, x, g))
    pi1, _ = mle(lambda x, g: ev_row(1, x, g))
    pip, iters = mle(joint(zero))
    ghat = ev_row(0, pi0, True)[1] + ev_row(1, pi1, True)[1]
    gpool = ev_row(0, pip, True)[1] + ev_row(1, pip, True)[1]
    stat = (2.0 * (ghat - gpool)).clamp_min(0.0)
    res = dict(pi0=pi0, pi1=pi1, pi_pool=pip, delta=pi1 - pi0, stat=stat, p_diff=torch.erfc((0.5 * stat).sqrt()).clamp_min(DBL_MIN), iters=iters)
    if interval:
        def profile(d, want_g):
            lo, hi = (-d).clamp_min(0.0), (1.0 - d).clamp_max(1.0)
            ev = joint(d)
            atlo = ev(lo, False)[0] <= 0
            athi = ~atlo & (ev(hi, False)[0] >= 0)
            x, _ = solve(ev, 0, ~atlo & ~athi, lo, hi, None)
            ps = torch.where(atlo, lo, torch.where(athi, hi, x))
            _, g0 = ev_row(0, ps, True)
            S1, g1 = ev_row(1, (ps + d).clamp(0.0, 1.0), True)
            return torch.where(atlo | athi, nan, S1), g0 + g1
        lo_end = 2.0 * (ghat - (ev_row(0, one, True)[1] + ev_row(1, zero, True)[1])) <= drop
        hi_end = 2.0 * (ghat - (ev_row(0, zero, True)[1] + ev_row(1, one, True)[1])) <= drop
        lo, _ = solve(profile, 1, ~lo_end, -one, res['delta'], ghat)
        hi, _ = solve(profile, 2, ~hi_end, res['delta'], one, ghat)
        res.update(delta_lo=torch.where(lo_end, -one, lo), delta_hi=torch.where(hi_end, one, hi))
    return res


def run(a):
    det = nm.DeviceDetector(0)
    rec = {'steps': a.steps, 'warmup': a.warmup, 'max_iter': 60, 'tol': 1e-12, 'shapes': []}
    for n, sites in SHAPES:
        sites = max(int(sites * a.scale), 64)
        note('drawing %d pairs of rows of %d scores' % (sites, n))
        s0, s1 = make_rows(sites, n, 1500 + n, 'cuda:0', 0.4), make_rows(sites, n, 2500 + n, 'cuda:0', 0.6)
        f0, f1 = s0.view(-1), s1.view(-1)
        kw = dict(stride0=n, stride1=n, npos=sites)
        full = det.site_diff(f0, f1, **kw)
        test = det.site_diff(f0, f1, interval=False, **kw)

        def three():
            k0 = det.site_stoich(f0, stride=n, npos=sites)
            k1 = det.site_stoich(f1, stride=n, npos=sites)
            kc = det.site_stoich(torch.cat((s0, s1), 1).view(-1), stride=2 * n, npos=sites)
            return (k0['stat'] + k1['stat'] - kc['stat']).clamp_min(0.0)
        stat3 = three()
        ref = torch_diff(s0, s1)
        torch.cuda.synchronize()
        ms = {'full': [], 'test': [], 'three': [], 'torch': []}
        for i in range(a.warmup + a.steps):                                     # alternated: all see the same machine state
            t = {'full': timed(lambda: det.site_diff(f0, f1, out=full, **kw))[0],
                 'test': timed(lambda: det.site_diff(f0, f1, interval=False, out=test, **kw))[0],
                 'three': timed(three)[0], 'torch': timed(lambda: torch_diff(s0, s1))[0]}
            note('n = %d: %s%s' % (n, ', '.join('%s %.3f ms' % kv for kv in t.items()), ' (warm-up)' if i < a.warmup else ''))
            if i >= a.warmup:
                for k, v in t.items():
                    ms[k].append(v)
        evals = int(full['iters'].sum())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        fin = torch.isfinite(stat3) & torch.isfinite(full['stat'])
        rec['shapes'].append({
            'scores_per_row': n, 'sites': sites, 'evaluations_for_pi_pool': evals,
            'estimates': int(((full['status'] & L.DIFF_NO_ESTIMATE) == 0).sum()), 'not_converged': int(((full['status'] & L.DIFF_NOT_CONVERGED) != 0).sum()),
            'ms_median': {k: round(v, 3) for k, v in med.items()}, 'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            'entry_sites_per_s': float('%.4g' % (sites / (med['full'] * 1e-3))),
            'entry_no_interval_sites_per_s': float('%.4g' % (sites / (med['test'] * 1e-3))),
            'entry_no_interval_scores_x_pool_evaluations_per_s': float('%.4g' % (2 * n * evals / (med['test'] * 1e-3))),
            'three_stoich_over_entry_no_interval': round(med['three'] / med['test'], 2), 'torch_over_entry': round(med['torch'] / med['full'], 2),
            'max_abs_diff_stat_three_calls': float((stat3 - full['stat'])[fin].abs().max()),
            'max_abs_diff_torch': {f: float((full[f] - ref[f]).abs().max()) for f in ('pi0', 'pi1', 'pi_pool', 'delta_lo', 'delta_hi', 'stat')}})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--scale', type=float, default=1.0, help='multiplies the number of sites of every shape')
    ap.add_argument('--write', default='', help='append the record to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_site_diff: no GPU; this measurement does not fall back')
    if a.steps < 3:
        sys.exit('bench_site_diff: the figure is a median of at least three steps')
    rec = run(a)
    rec['build'] = L.load().nmod_build_info().decode()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.write:
        with open(a.write, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
