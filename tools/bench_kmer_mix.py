#!/usr/bin/env python3
"""Side measurement of nmod_kmer_mix (K17) on one GPU, not the headline bench: DeviceDetector.kmer_mix on event-like int16 rows of
nmod_synth_fill_events with k = 5 and 6 (1 024 and 4 096 codes) at 4.6 M x 200 and at the configs[4] ragged sizes, against the control
table nmod_kmer_model gives for the same rows — and, in the same process on the same rows, the route the tree offered for the same
numbers before the entry existed: a torch.bincount into the same windows plus the same EM in torch tensor operations (every code
runs as many iterations as the entry's slowest code; no per-code stopping).

Each call is timed by its own pair of HIP events after a warm-up; the figure is the median.  The histogram pass is timed apart from
the EM by a second call with max_iter = 1 (the grouping, the histogram pass and one EM iteration).  The bytes are what the algorithm
has to read: the samples once, 8 bytes of offsets (CSR) and 4 of code per position.  One JSON line per leg; --write FILE also writes
the record kept as profiles/kmer_mix.txt.

    python tools/bench_kmer_mix.py [--steps 10] [--warmup 2] [--legs 200,ragged] [--ks 5,6] [--scale 1.0] [--write profiles/kmer_mix.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nanomod_amd as nm

L = nm._lib
DEV = 'cuda:0'
HBM_PEAK = 8.0e12                             # bytes / s: the data-sheet rate
MAX_ITER, TOL = 50, 1e-6


def timed_median(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def torch_route(sig, n_per_row, codes, ncodes, mean0, sd0, iters):
    """the parent's route: the histogram by torch.bincount, `iters` EM iterations (free variance) over all codes at once"""
    usable = torch.isfinite(mean0) & torch.isfinite(sd0) & (sd0 > 0) & (mean0.abs() <= 1000.0)
    lo = torch.where(usable, torch.round(1000.0 * torch.nan_to_num(mean0)), torch.zeros_like(mean0)).to(torch.int64) - L.KMIX_HALF
    take = (codes >= 0) & usable[codes.clamp(min=0).long()]
    c = torch.repeat_interleave(torch.where(take, codes, torch.full_like(codes, -1)).long(), n_per_row)
    b = sig.long() - lo[c.clamp(min=0)]
    inside = (c >= 0) & (b >= 0) & (b < L.KMIX_BINS)
    hist = torch.bincount((c * L.KMIX_BINS + b)[inside], minlength=ncodes * L.KMIX_BINS).view(ncodes, L.KMIX_BINS)
    del c, b, inside
    h = hist.double()
    n = h.sum(1)
    x = (lo[:, None] + torch.arange(L.KMIX_BINS, device=sig.device)[None, :]).double() / 1000.0
    mu, s2 = mean0[:, None], (sd0 * sd0)[:, None]
    ybar = (h * x).sum(1) / n
    pi, m, v = torch.full_like(n, 0.5)[:, None], (mean0 + 2.0 * (ybar - mean0))[:, None], s2.clone()
    a = (x - mu) ** 2 / (2.0 * s2)
    for _ in range(iters):
        t = torch.log((1.0 - pi) / pi) + 0.5 * torch.log(v / s2) + (x - m) ** 2 / (2.0 * v) - a
        r = h / (1.0 + torch.exp(t))
        w = r.sum(1, keepdim=True)
        pi, m = w / n[:, None], (r * x).sum(1, keepdim=True) / w
        v = torch.maximum((r * (x - m) ** 2).sum(1, keepdim=True) / w, s2 / 16.0)
    return hist, pi[:, 0], m[:, 0], torch.sqrt(v[:, 0])


def leg(name, k, npos, n, steps, warmup, off=None, seed=7):
    det = nm.DeviceDetector(0)
    ncodes = 4 ** k
    total = int(off[-1]) if off is not None else npos * n
    doff = torch.from_numpy(off).to(DEV) if off is not None else None
    sig = torch.empty(total, dtype=torch.int16, device=DEV)
    det.synth_fill_events(sig, seed, 0, npos, 0, n_per_pos=0 if off is not None else n, off=doff)
    codes = torch.randint(0, ncodes, (npos,), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    stride = 0 if off is not None else n
    ctl = det.kmer_model(sig, codes, ncodes, off=doff, stride=stride)
    mean0, sd0 = ctl['mean'], ctl['sd']
    kw = dict(off=doff, stride=stride, model='free', tol=TOL)
    out = det.kmer_mix(sig, codes, ncodes, mean0, sd0, max_iter=MAX_ITER, want_hist=True, **kw)
    ms, lo, hi = timed_median(lambda: det.kmer_mix(sig, codes, ncodes, mean0, sd0, max_iter=MAX_ITER, want_hist=True, out=out, **kw), steps, warmup)
    one = det.kmer_mix(sig, codes, ncodes, mean0, sd0, max_iter=1, **kw)
    ms1, _, _ = timed_median(lambda: det.kmer_mix(sig, codes, ncodes, mean0, sd0, max_iter=1, out=one, **kw), steps, warmup)
    iters = int(out['iters'].max())
    n_per_row = torch.diff(doff) if off is not None else torch.full((npos,), n, dtype=torch.int64, device=DEV)
    route = lambda: torch_route(sig, n_per_row, codes, ncodes, mean0, sd0, iters)
    p_ms, _, _ = timed_median(route, max(steps // 3, 3), 1)
    hist, pi, m, sd = route()
    torch.cuda.synchronize()
    done = ((out['status'] & L.KMIX_NO_ESTIMATE) == 0) & (out['iters'] == iters)    # the codes that ran the torch route's iteration count
    nbytes = total * 2 + (8 * (npos + 1) if off is not None else 0) + 4 * npos
    rate = nbytes / (ms1 * 1e-3)
    rec = {'leg': name, 'k': k, 'codes': ncodes, 'positions': npos, 'samples': total, 'bytes': nbytes, 'bytes_per_position': nbytes / npos,
           'kmer_mix_ms': ms, 'kmer_mix_ms_min': lo, 'kmer_mix_ms_max': hi, 'steps': steps, 'max_iter': MAX_ITER, 'iters_max': iters,
           'kmer_mix_one_iteration_ms': ms1, 'hist_pass_GBps_at_least': rate / 1e9, 'of_8TBps': rate / HBM_PEAK,
           'torch_route_ms': p_ms, 'torch_over_kmer_mix': p_ms / ms,
           'hist_equal': bool(torch.equal(hist.to(torch.int32), out['hist'].view(ncodes, L.KMIX_BINS))),
           'compared_codes': int(done.sum()),
           'max_abs_diff_pi': float((out['pi'] - pi)[done].abs().max()) if bool(done.any()) else None,
           'max_abs_diff_mu': float((out['mu_mod'] - m)[done].abs().max()) if bool(done.any()) else None}
    print(json.dumps(rec), flush=True)
    return rec


def write_record(path, recs):
    with open(path, 'w') as f:
        f.write('nmod_kmer_mix (K17) — measurements\n')
        f.write('==================================\n\n')
        f.write('tools/bench_kmer_mix.py on one MI355X: int16 rows of nmod_synth_fill_events, random codes, the control table from\n')
        f.write('nmod_kmer_model on the same rows; free variance, max_iter %d, tol %g; HIP events around each call, median of `steps`\n' % (MAX_ITER, TOL))
        f.write('after a warm-up.  bytes = samples + 8 per position of offsets (CSR legs) + 4 per position of code.  "one iteration" is the\n')
        f.write('whole entry with max_iter = 1: the grouping, the histogram pass and one EM iteration, so the rate given for the histogram\n')
        f.write('pass is a lower bound.  torch route = torch.bincount into the same windows + the same EM in torch tensor operations, every\n')
        f.write('code running the entry\'s largest iteration count.\n\n')
        for r in recs:
            f.write('   %s, k = %d (%d codes): %d positions, %d samples, %.1f bytes per position\n'
                    % (r['leg'], r['k'], r['codes'], r['positions'], r['samples'], r['bytes_per_position']))
            f.write('     nmod_kmer_mix    %.3f ms (min %.3f, max %.3f, %d calls; largest iteration count %d)\n'
                    % (r['kmer_mix_ms'], r['kmer_mix_ms_min'], r['kmer_mix_ms_max'], r['steps'], r['iters_max']))
            f.write('     one iteration    %.3f ms   >= %.1f GB/s = %.3f of 8 TB/s for the histogram pass\n'
                    % (r['kmer_mix_one_iteration_ms'], r['hist_pass_GBps_at_least'], r['of_8TBps']))
            f.write('     torch route      %.1f ms   ratio %.1f x   histogram equal: %s; over the %d codes of that iteration count |pi diff| <= %s, |mu_mod diff| <= %s\n'
                    % (r['torch_route_ms'], r['torch_over_kmer_mix'], r['hist_equal'], r['compared_codes'],
                       '%.2e' % r['max_abs_diff_pi'] if r['max_abs_diff_pi'] is not None else 'n/a',
                       '%.2e' % r['max_abs_diff_mu'] if r['max_abs_diff_mu'] is not None else 'n/a'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--legs', default='200,ragged')
    ap.add_argument('--ks', default='5,6')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the positions of every leg')
    ap.add_argument('--write', default='', help='write the record (profiles/kmer_mix.txt) here')
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: the median is of at least 10 calls')
    legs, ks = a.legs.split(','), [int(k) for k in a.ks.split(',')]
    sc = lambda p: max(int(p * a.scale), 1024)
    recs = []
    if '200' in legs:
        for k in ks:
            recs.append(leg('4.6M x 200', k, sc(4_600_000), 200, a.steps, a.warmup))
    if 'ragged' in legs:                       # the group-1 sizes of BASELINE.json configs[4]: LogNormal(ln 1000, 0.5) in [5, 4000]
        P = sc(1_000_000)
        n0 = np.clip(np.round(np.random.default_rng(5).lognormal(np.log(1000), 0.5, P)), 5, 4000).astype(np.int64)
        off = np.zeros(P + 1, np.int64); off[1:] = np.cumsum(n0)
        for k in ks:
            recs.append(leg('configs[4] ragged ~1000', k, P, 1000, a.steps, a.warmup, off=off))
    if a.write:
        write_record(a.write, recs)


if __name__ == '__main__':
    main()
