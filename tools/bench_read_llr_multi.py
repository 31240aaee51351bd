#!/usr/bin/env python3
"""Side measurement of K26 on one GPU, not the headline bench.

1. nmod_read_llr_multi at n_alt = 2 and 4 against n_alt separate nmod_read_llr calls (K13's entry, unchanged) on the same int16 events,
   for both table placements (k = 3: the table in LDS; k = 5: through L2), alternated in one loop so that both see the same machine
   state.  Both are asked for llr_win alone (the multi call for `call` as well: it cannot be had from separate calls).  The streaming
   bound of the fused call is the element's bytes + 1 read per event and 8 n_alt + 1 B written; of the separate calls n_alt times
   (element + 1 + 8).
2. nmod_site_compose in rows / s for the three size classes (rows of 40, 600 and 2 000 reads, n_alt = 2 and 4), the per-state test on.

Each call is timed by its own pair of HIP events after a warm-up; a figure is the median of `steps` calls.  One JSON line per run;
--write-multi / --write-compose append the records kept in profiles/read_llr_multi.txt and profiles/site_compose.txt.

    python tools/bench_read_llr_multi.py [--steps 5] [--warmup 2] [--reads 4000] [--events 5000] [--write-multi FILE] [--write-compose FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
import nanomod_amd as nm
from bench_read_calls import make_reads, timed, summary, HBM_PEAK

L = nm._lib
DEV = 'cuda:0'
_T0 = time.time()


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def bench_multi(a, det, k, n_alt):
    center, thr = k // 2, 2.5
    g = torch.Generator(DEV).manual_seed(260 + k)
    nc = 4 ** k
    mean = torch.randn(nc, dtype=torch.float64, device=DEV, generator=g)
    sd = torch.rand(nc, dtype=torch.float64, device=DEV, generator=g) * 0.2 + 0.1
    alt_means = [mean + (torch.rand(nc, dtype=torch.float64, device=DEV, generator=g) * 6.0 - 3.0) * sd for _ in range(n_alt)]
    alt_sds = [sd * (torch.rand(nc, dtype=torch.float64, device=DEV, generator=g) * 1.5 + 0.5) for _ in range(n_alt)]
    off_host = np.arange(a.reads + 1, dtype=np.int64) * a.events
    total = int(off_host[-1])
    off, val, base = make_reads(off_host, mean, sd, k, center, 11)
    torch.cuda.synchronize()
    want = ('llr_win', 'call')
    fused = lambda out=None: det.read_llr_multi(val, off, base, mean, sd, alt_means, alt_sds, k, center, thr=thr, want=want, out=out)
    out_f = fused()
    outs = [det.read_llr(val, off, base, mean, sd, alt_means[m], alt_sds[m], k, center, thr=thr, want=('llr_win',)) for m in range(n_alt)]
    torch.cuda.synchronize()
    same = all(torch.equal(out_f['llr_win'][m].view(torch.int64), outs[m]['llr_win'].view(torch.int64)) for m in range(n_alt))

    def separate():
        for m in range(n_alt):
            det.read_llr(val, off, base, mean, sd, alt_means[m], alt_sds[m], k, center, thr=thr, want=('llr_win',), out=outs[m])
    ms_f, ms_s = [], []
    for i in range(a.warmup + a.steps):                                         # alternated: both see the same machine state
        tf, _ = timed(lambda: fused(out_f))
        ts, _ = timed(separate)
        note('k=%d n_alt=%d: fused %.3f ms, %d separate calls %.3f ms%s' % (k, n_alt, tf, n_alt, ts, ' (warm-up)' if i < a.warmup else ''))
        if i >= a.warmup:
            ms_f.append(tf); ms_s.append(ts)
    esz = val.element_size()
    sf, ss = summary(ms_f, total), summary(ms_s, total)
    sf.update(streaming_bytes_per_event=esz + 1 + 8 * n_alt + 1, share_of_8TBps=round(sf['events_per_s'] * (esz + 1 + 8 * n_alt + 1) / HBM_PEAK, 5))
    ss.update(streaming_bytes_per_event=n_alt * (esz + 1 + 8), share_of_8TBps=round(ss['events_per_s'] * n_alt * (esz + 1 + 8) / HBM_PEAK, 5))
    return {'k': k, 'n_alt': n_alt, 'table_in_lds': bool(L.load().nmod_read_llr_multi_table_in_lds(n_alt, k)), 'events': total, 'planes_bit_equal': same,
            'fused': sf, 'separate': ss, 'separate_over_fused': round(float(np.median(ms_s)) / float(np.median(ms_f)), 3)}


def bench_compose(a, det, n_alt, n, rows):
    rng = np.random.default_rng(2600 + n)
    shares = np.array([0.5] + [0.5 / n_alt] * n_alt)
    z = rng.choice(n_alt + 1, size=(rows, n), p=shares)
    y = rng.normal(size=(n_alt, rows, n))
    for m in range(1, n_alt + 1):
        y[m - 1] += 2.0 * (z == m)
    scores = [torch.from_numpy(np.ascontiguousarray((2.0 * y[m] - 2.0).reshape(-1))).to(DEV) for m in range(n_alt)]
    call = lambda out=None: det.site_compose(scores, stride=n, out=out)
    out = call()
    torch.cuda.synchronize()
    ms = []
    for i in range(a.warmup + a.steps):
        t, _ = timed(lambda: call(out))
        note('site_compose n_alt=%d rows of %d: %.3f ms%s' % (n_alt, n, t, ' (warm-up)' if i < a.warmup else ''))
        if i >= a.warmup:
            ms.append(t)
    med = float(np.median(ms))
    return {'n_alt': n_alt, 'reads_per_row': n, 'rows': rows, 'ms_median': round(med, 4), 'ms_all': [round(v, 4) for v in ms],
            'rows_per_s': round(rows / (med * 1e-3), 1), 'mean_iters': round(float(out['iters'].double().mean()), 2),
            'not_converged': int((out['status'] & L.COMPOSE_NOT_CONVERGED).ne(0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--events', type=int, default=5000)
    ap.add_argument('--write-multi', default='', help='append the read_llr_multi record to this file')
    ap.add_argument('--write-compose', default='', help='append the site_compose record to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_llr_multi: no GPU; this measurement does not fall back')
    if a.steps < 3:
        sys.exit('bench_read_llr_multi: the figure is a median of at least three steps')
    det = nm.DeviceDetector(0)
    build = L.load().nmod_build_info().decode()
    multi = {'what': 'read_llr_multi against separate read_llr calls', 'dtype': 'int16', 'window': 'kmer', 'steps': a.steps, 'warmup': a.warmup,
             'cases': [bench_multi(a, det, k, n_alt) for k in (3, 5) for n_alt in (2, 4)], 'build': build}
    compose = {'what': 'site_compose rows per second', 'steps': a.steps, 'warmup': a.warmup, 'opts': 'defaults (min_valid 3, max_iter 500, tol 1e-9), test on',
               'cases': [bench_compose(a, det, n_alt, n, rows) for n_alt in (2, 4) for n, rows in ((40, 200000), (600, 20000), (2000, 4000))], 'build': build}
    for rec, path in ((multi, a.write_multi), (compose, a.write_compose)):
        line = json.dumps(rec)
        print(line, flush=True)
        if path:
            with open(path, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
