#!/usr/bin/env python3
"""Side measurement of nmod_read_llr (K13) on one GPU, not the headline bench: DeviceDetector.read_llr on int16 reads drawn from a
k-mer model on the device, alternated in one loop with nmod_read_calls (K12) asked for p_win alone on the same input, so that both see
the same machine state.  K12 is the yardstick: K13 does strictly less arithmetic per event.

Each call is timed by its own pair of HIP events after a warm-up; the figure is the median of `steps` calls (three by default).  The
streaming bound is the element's bytes + 1 read per event and 8 B written per requested track: 11 B for one track of int16 events,
27 B for three.  One JSON line per run; --write FILE appends the record kept in profiles/read_llr.txt.

    python tools/bench_read_llr.py [--steps 3] [--warmup 1] [--reads 4000] [--events 5000] [--kmer 5] [--window kmer|LO,HI] [--write FILE]
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
from bench_read_calls import make_reads, timed, summary, HBM_PEAK, HBM_COPY

L = nm._lib
DEV = 'cuda:0'
_T0 = time.time()


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def run(a):
    k, center, thr = a.kmer, a.kmer // 2, 2.5
    window = 'kmer' if a.window == 'kmer' else tuple(int(v) for v in a.window.split(','))
    lo, hi = (k - 1 - center, center) if window == 'kmer' else window
    nb12 = max(lo, hi)                                                          # K12's window is symmetric: the wider side
    g = torch.Generator(DEV).manual_seed(100 + k)
    mean = torch.randn(4 ** k, dtype=torch.float64, device=DEV, generator=g)
    sd = torch.rand(4 ** k, dtype=torch.float64, device=DEV, generator=g) * 0.2 + 0.1
    alt_mean = mean + (torch.rand(4 ** k, dtype=torch.float64, device=DEV, generator=g) * 6.0 - 3.0) * sd
    alt_sd = sd * (torch.rand(4 ** k, dtype=torch.float64, device=DEV, generator=g) * 1.5 + 0.5)
    off_host = np.arange(a.reads + 1, dtype=np.int64) * a.events
    total = int(off_host[-1])
    note('drawing', total, 'events')
    off, val, base = make_reads(off_host, mean, sd, k, center, 11)
    torch.cuda.synchronize()
    det = nm.DeviceDetector(0)
    rec = {'dtype': 'int16', 'k': k, 'center': center, 'window': [lo, hi], 'thr': thr, 'k12_nb': nb12, 'reads': a.reads, 'events': total,
           'steps': a.steps, 'warmup': a.warmup}
    out12 = det.read_calls(val, off, base, mean, sd, k, center, nb=nb12, alpha=0.01, want=('p_win',))
    for want in (('llr_win',), L.LLR_EVENT_FIELDS):
        nbytes = val.element_size() + 1 + 8 * len(want)
        out13 = det.read_llr(val, off, base, mean, sd, alt_mean, alt_sd, k, center, window=window, thr=thr, want=want)
        torch.cuda.synchronize()
        ms13, ms12 = [], []
        for i in range(a.warmup + a.steps):                                     # alternated: both see the same machine state
            t13, _ = timed(lambda: det.read_llr(val, off, base, mean, sd, alt_mean, alt_sd, k, center, window=window, thr=thr, want=want, out=out13))
            t12, _ = timed(lambda: det.read_calls(val, off, base, mean, sd, k, center, nb=nb12, alpha=0.01, want=('p_win',), out=out12))
            note('want=%s: K13 %.3f ms, K12 p_win %.3f ms%s' % ('+'.join(want), t13, t12, ' (warm-up)' if i < a.warmup else ''))
            if i >= a.warmup:
                ms13.append(t13)
                ms12.append(t12)
        s = summary(ms13, total)
        s.update(streaming_bytes_per_event=nbytes, share_of_8TBps=round(s['events_per_s'] * nbytes / HBM_PEAK, 5),
                 share_of_measured_copy_6p29TBps=round(s['events_per_s'] * nbytes / HBM_COPY, 5))
        s12 = summary(ms12, total)
        s12.update(streaming_bytes_per_event=11, share_of_8TBps=round(s12['events_per_s'] * 11 / HBM_PEAK, 5))
        rec['k13_' + '_'.join(want)] = s
        rec['k12_p_win_beside_' + '_'.join(want)] = s12
        rec['k13_over_k12_' + '_'.join(want)] = round(float(np.median(ms12)) / float(np.median(ms13)), 2)
    rec['scored_events'] = int(out13['n_sites'].sum())
    rec['mod_events'] = int(out13['n_mod'].sum())
    rec['can_events'] = int(out13['n_can'].sum())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--events', type=int, default=5000)
    ap.add_argument('--kmer', type=int, default=5)
    ap.add_argument('--window', default='kmer', help="'kmer' or LO,HI")
    ap.add_argument('--write', default='', help='append the record to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_llr: no GPU; this measurement does not fall back')
    if a.steps < 3:
        sys.exit('bench_read_llr: the figure is a median of at least three steps')
    rec = run(a)
    rec['build'] = L.load().nmod_build_info().decode()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.write:
        with open(a.write, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
