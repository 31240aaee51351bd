#!/usr/bin/env python3
"""Side measurement of nmod_site_stoich (K14) on one GPU, not the headline bench: DeviceDetector.site_stoich on fixed-stride rows of
simulated window sums, alternated in one loop with the same definition written in torch tensor operations (all rows at once, a mask for
the rows that have stopped, one host read per evaluation to see whether any row still runs), so that both see the same machine state.

Rows of 30 and 200 scores (the 16-lane form), 600 (the wave form) and 2 000 (the workgroup form).  Each call is timed by its own pair
of HIP events after a warm-up; the figure is the median of `steps` calls (three at least).  Reported per row length: rows/s, scores x evaluations/s
(the evaluations of the iteration for pi^ as the entry counts them in `iters`, the two ends and the interval roots not counted), the
ratio torch / entry, and the largest difference of pi^ between the two routes.  One JSON line per run; --write FILE appends the record
kept in profiles/site_stoich.txt.

    python tools/bench_site_stoich.py [--steps 3] [--warmup 1] [--scale 1.0] [--write FILE]
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
SHAPES = ((30, 400000), (200, 100000), (600, 30000), (2000, 10000))      # (scores per row, rows): 12, 20, 18 and 20 million scores


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def make_rows(rows, n, seed, device):
    """window sums at positions where a share of 0 .. 0.6 is modified, the two levels 2 sd apart"""
    g = torch.Generator(device).manual_seed(seed)
    share = torch.rand(rows, 1, dtype=torch.float64, device=device, generator=g) * 0.6
    z = (torch.rand(rows, n, dtype=torch.float64, device=device, generator=g) < share).to(torch.float64)
    x = torch.randn(rows, n, dtype=torch.float64, device=device, generator=g) + 2.0 * z
    return (2.0 * x - 2.0).contiguous()


def torch_stoich(s, max_iter=60, tol=1e-12, drop=L.STOICH_CI_DROP_95):
    """include/nanomod_hip.h's definition of nmod_site_stoich over the rows of a matrix of valid scores, in tensor operations"""
    t = -torch.expm1(-s.abs())
    plus = s >= 0

    def evaluate(pi, want_g):
        qt = torch.where(plus, (1.0 - pi)[:, None], pi[:, None]) * t
        u = t / (1.0 - qt)
        S = torch.where(plus, u, -u).sum(1)
        return S, (torch.log1p(-qt).sum(1) if want_g else (u * u).sum(1))

    def solve(mode, run, a, b, ghat):
        a, b = a.clone(), b.clone()
        x = a + 0.5 * (b - a)
        active = run.clone()
        iters = torch.zeros_like(x, dtype=torch.int32)
        for k in range(1, max_iter + 1):
            if not bool(active.any()):
                break
            S, X = evaluate(x, mode != 0)
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

    zero, one = torch.zeros(s.shape[0], dtype=s.dtype, device=s.device), torch.ones(s.shape[0], dtype=s.dtype, device=s.device)
    S0, g0 = evaluate(zero, True)
    S1, g1 = evaluate(one, True)
    at0 = S0 <= 0
    at1 = ~at0 & (S1 >= 0)
    x, iters = solve(0, ~at0 & ~at1, zero, one, None)
    pi = torch.where(at0, zero, torch.where(at1, one, x))
    _, gh = evaluate(pi, True)
    lhat = torch.where(at0, zero, (gh + torch.where(plus, s, torch.zeros_like(s)).sum(1)).clamp_min(0.0))
    lo0, hi1 = 2.0 * (gh - g0) <= drop, 2.0 * (gh - g1) <= drop
    lo, _ = solve(1, ~lo0, zero, pi, gh)
    hi, _ = solve(2, ~hi1, pi, one, gh)
    p_null = torch.where(at0, one, (0.5 * torch.erfc(lhat.sqrt())).clamp_min(2.2250738585072014e-308))
    return dict(pi=pi, pi_lo=torch.where(lo0, zero, lo), pi_hi=torch.where(hi1, one, hi), stat=2.0 * lhat, p_null=p_null, iters=iters)


def run(a):
    det = nm.DeviceDetector(0)
    rec = {'steps': a.steps, 'warmup': a.warmup, 'max_iter': 60, 'tol': 1e-12, 'shapes': []}
    for n, rows in SHAPES:
        rows = max(int(rows * a.scale), 64)
        note('drawing %d rows of %d scores' % (rows, n))
        s = make_rows(rows, n, 1400 + n, 'cuda:0')
        flat = s.view(-1)
        out = det.site_stoich(flat, stride=n, npos=rows)
        ref = torch_stoich(s)
        torch.cuda.synchronize()
        ms_k, ms_t = [], []
        for i in range(a.warmup + a.steps):                                     # alternated: both see the same machine state
            tk, _ = timed(lambda: det.site_stoich(flat, stride=n, npos=rows, out=out))
            tt, ref = timed(lambda: torch_stoich(s))
            note('n = %d: entry %.3f ms, torch %.3f ms%s' % (n, tk, tt, ' (warm-up)' if i < a.warmup else ''))
            if i >= a.warmup:
                ms_k.append(tk)
                ms_t.append(tt)
        evals = int(out['iters'].sum())
        mk, mt = float(np.median(ms_k)), float(np.median(ms_t))
        rec['shapes'].append({
            'scores_per_row': n, 'rows': rows, 'evaluations_for_pi': evals, 'estimates': int(((out['status'] & L.STOICH_NO_ESTIMATE) == 0).sum()),
            'entry_ms_median': round(mk, 3), 'entry_ms_min_max': [round(min(ms_k), 3), round(max(ms_k), 3)],
            'torch_ms_median': round(mt, 3), 'torch_ms_min_max': [round(min(ms_t), 3), round(max(ms_t), 3)],
            'entry_rows_per_s': float('%.4g' % (rows / (mk * 1e-3))), 'entry_scores_x_evaluations_per_s': float('%.4g' % (n * evals / (mk * 1e-3))),
            'torch_rows_per_s': float('%.4g' % (rows / (mt * 1e-3))), 'torch_over_entry': round(mt / mk, 2),
            'max_abs_diff_pi': float((out['pi'] - ref['pi']).abs().max()), 'max_abs_diff_pi_lo': float((out['pi_lo'] - ref['pi_lo']).abs().max()),
            'max_abs_diff_pi_hi': float((out['pi_hi'] - ref['pi_hi']).abs().max()),
            'max_rel_diff_stat': float(((out['stat'] - ref['stat']).abs() / ref['stat'].abs().clamp_min(1.0)).max())})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--scale', type=float, default=1.0, help='multiplies the number of rows of every shape')
    ap.add_argument('--write', default='', help='append the record to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_site_stoich: no GPU; this measurement does not fall back')
    if a.steps < 3:
        sys.exit('bench_site_stoich: the figure is a median of at least three steps')
    rec = run(a)
    rec['build'] = L.load().nmod_build_info().decode()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.write:
        with open(a.write, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
