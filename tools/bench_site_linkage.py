#!/usr/bin/env python3
"""Side measurement of the soft linkage of site pairs (K18) on one GPU, not the headline bench.

--part rows: DeviceDetector.pair_rows (nmod_pair_rows_count + nmod_pair_rows_fill: two walks over the reads, the scan, the sort of the
  row keys, the gather; one synchronisation in the middle, so the figure is host wall time between two stream synchronisations, not
  an event pair) beside DeviceDetector.site_pairs asked for the counts alone (K16's one walk) on the same reads, alternated in one
  loop.  Shapes: bench_site_pairs.py's coverage 30 over 10^4 sites and coverage 1 000 over 10^3 sites, window sums drawn from two
  levels 2 sd apart (every score valid).  Reported: reads/s and rows/s.
--part link: DeviceDetector.pair_linkage alone (HIP events) over rows of one length per shape: 30, 100 and 250 reads (the 16-lane form),
  300 and 1 000 (the wave), 1 500 and 5 000 (the workgroup), levels 2 sd apart, shares 0.3 / 0.4, D 0.05; with and without the interval.
  Reported: pairs/s, reads/s, and the median number of evaluations of the root of D.

The figure is the median of `steps` calls after a warm-up, the spread their minimum and maximum.  One JSON line per row; --write FILE
appends them.

    python tools/bench_site_linkage.py --part rows|link [--steps 5] [--warmup 1] [--write FILE]
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


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def timed_events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def timed_wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def soft_scores(n, sep, share, g, dev):
    """window sums of n events, a share of them from the modified level: s = sep x - sep^2 / 2"""
    z = torch.rand(n, device=dev, generator=g, dtype=torch.float64) < share
    x = torch.randn(n, device=dev, generator=g, dtype=torch.float64) + sep * z
    return sep * x - 0.5 * sep * sep


def part_rows(a, det, dev):
    rows = []
    for name, nreads, read_len, span, nsites in (('coverage 30, 10^4 sites', 3000, 1000, 100000, 10000),
                                                 ('coverage 1000, 10^3 sites', 10000, 1000, 10000, 1000)):
        g = torch.Generator(dev).manual_seed(7)
        start = torch.randint(0, span - read_len + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
        cs = torch.randint(0, 2, (nreads,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
        score = soft_scores(nreads * read_len, 2.0, 0.3, g, dev)
        pos = torch.arange(nsites, device=dev, dtype=torch.int64) * 10
        key = torch.cat([pos, (1 << 40) | pos])
        poff, npairs = det.pair_index(key, 100)
        args = (cs, start, roff, score, key, poff, npairs)
        routes = dict(rows=lambda: det.pair_rows(*args), counts=lambda: det.site_pairs(*args, thr=2.5, want=('counts',)))
        ms = {r: [] for r in routes}
        out = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out[r] = timed_wall(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        nrows = int(out['rows']['sa'].numel())
        row = dict(part='rows', shape=name, reads=nreads, events=nreads * read_len, sites=2 * nsites, pairs=npairs, nrows=nrows,
                   **{r: spread(v) for r, v in ms.items()})
        row['rows']['reads_per_s'] = nreads / (row['rows']['median'] / 1e3)
        row['rows']['rows_per_s'] = nrows / (row['rows']['median'] / 1e3)
        row['counts']['reads_per_s'] = nreads / (row['counts']['median'] / 1e3)
        note(json.dumps(row))
        rows.append(row)
        del out
    return rows


def part_link(a, det, dev):
    rows = []
    for n, npairs in ((30, 200000), (100, 100000), (250, 40000), (300, 40000), (1000, 10000), (1500, 4000), (5000, 1000)):
        g = torch.Generator(dev).manual_seed(11)
        # the joint law (0.3, 0.4, D = 0.05): the state of site b given that of site a
        za = torch.rand(n * npairs, device=dev, generator=g, dtype=torch.float64) < 0.3
        pb = torch.where(za, (0.3 * 0.4 + 0.05) / 0.3, (0.7 * 0.4 - 0.05) / 0.7)
        zb = torch.rand(n * npairs, device=dev, generator=g, dtype=torch.float64) < pb
        sa = 2.0 * (torch.randn(n * npairs, device=dev, generator=g, dtype=torch.float64) + 2.0 * za) - 2.0
        sb = 2.0 * (torch.randn(n * npairs, device=dev, generator=g, dtype=torch.float64) + 2.0 * zb) - 2.0
        off = torch.arange(npairs + 1, device=dev, dtype=torch.int64) * n
        routes = dict(all=lambda: det.pair_linkage(sa, sb, off), no_interval=lambda: det.pair_linkage(sa, sb, off, interval=False))
        ms = {r: [] for r in routes}
        out = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out[r] = timed_events(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        form = '16 lanes' if n <= L.LINK_SMALL else ('wave' if n <= L.LINK_WAVE else 'workgroup')
        row = dict(part='link', form=form, reads_per_pair=n, pairs=npairs, iters_median=int(out['all']['iters'].median()),
                   estimated=int(((out['all']['status'] & L.LINK_NO_ESTIMATE) == 0).sum()), d_mean=float(out['all']['d'].nanmean()),
                   **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            row[r]['pairs_per_s'] = npairs / (row[r]['median'] / 1e3)
            row[r]['reads_per_s'] = npairs * n / (row[r]['median'] / 1e3)
        note(json.dumps(row))
        rows.append(row)
        del sa, sb, out
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['rows', 'link'], required=True)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--write', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_site_linkage: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    note(L.load().nmod_build_info().decode())
    rows = part_rows(a, det, dev) if a.part == 'rows' else part_link(a, det, dev)
    for row in rows:
        print(json.dumps(row))
    if a.write:
        with open(a.write, 'a') as f:
            f.writelines(json.dumps(row) + '\n' for row in rows)


if __name__ == '__main__':
    main()
