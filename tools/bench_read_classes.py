#!/usr/bin/env python3
"""Side measurement of the latent-class clustering of reads (K22) on one GPU, not the headline bench.

Per shape: one DeviceDetector.read_classes_step (nmod_read_classes_step: E-step, M-step, the weights and sums) with C = 2 and with
C = 8 classes, the DeviceDetector.read_class_rows call that prepares a data set (nmod_read_class_rows: the entries, the sort by site),
and a whole 2-class fit (readllr.fit_classes from one seeded start, `sums` read back per step), alternated IN THE SAME LOOP with
DeviceDetector.read_hmm with every output (K19's full forward-backward call) on the same entries, so that the comparison is against K19
on the same run, the same data and the same clocks.  HIP events around every call.  Shapes: every tenth position a candidate site; the
reads of two planted classes, one modified at 0.8 of the sites of the first half of the reference and at 0.1 of the second, the other
the reverse; window sums 2 sd apart:
  many rows a site   reads of 2 000 events (200 entries) over a reference of 8 000 positions: every site a workgroup's,
  few rows a site    the same reads over 800 000 positions: sites of the 16-lane form,
  long reads         reads of 20 000 events (2 000 entries, the workgroup form of the E-step) over 80 000 positions.
Reported: rows/s and the ratio to K19's call.  The figure is the median of `steps` calls after a warm-up, the spread their minimum and
maximum.  One JSON line per row; --write FILE appends them.

    python tools/bench_read_classes.py [--steps 5] [--warmup 1] [--write FILE]
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
from nanomod_amd import readllr

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


def spread(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--write', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_classes: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    note(L.load().nmod_build_info().decode())
    out_rows = []
    for name, read_len, nreads, span in (('many rows a site', 2000, 20000, 8000), ('few rows a site', 2000, 20000, 800000),
                                         ('long reads', 20000, 2000, 80000)):
        g = torch.Generator(dev).manual_seed(22)
        start = torch.randint(0, span - read_len + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
        cs = torch.zeros(nreads, device=dev, dtype=torch.int32)
        roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
        pos = (start[:, None] + torch.arange(read_len, device=dev)[None, :]).reshape(-1)
        cls = (torch.arange(nreads, device=dev) % 3 == 0).repeat_interleave(read_len)
        share = torch.where((pos < span // 2) == cls, 0.8, 0.1)
        z = torch.rand(nreads * read_len, device=dev, generator=g, dtype=torch.float64) < share
        score = 2.0 * (torch.randn(nreads * read_len, device=dev, generator=g, dtype=torch.float64) + 2.0 * z) - 2.0
        del pos, cls, share, z
        key = torch.arange(span // 10, device=dev, dtype=torch.int64) * 10
        args = (cs, start, roff, score, key)
        (hoff, nrows) = det.read_sites(*args)
        rows = det.read_class_rows(*args, hoff, nrows)
        nsites = int(key.numel())
        par = {}
        for nc in (2, 8):
            th = torch.from_numpy(readllr.class_starts(np.full(nsites, 0.4), nc, 1, 22)[0].reshape(-1)).to(dev)
            par[nc] = (th, torch.full((nc,), 1.0 / nc, dtype=torch.float64, device=dev))

        def fit():
            def step(theta, w):
                res = det.read_classes_step(rows, hoff, theta, w, want=('theta_out', 'w_out', 'sums'))
                return res['theta_out'], res['w_out'], res['sums'].cpu().tolist()
            return readllr.fit_classes(step, *par[2])
        routes = dict(k19_all=lambda: det.read_hmm(*args, hoff, nrows, pi=0.33, length=2000.0),
                      step_c2=lambda: det.read_classes_step(rows, hoff, *par[2]),
                      step_c8=lambda: det.read_classes_step(rows, hoff, *par[8]),
                      class_rows=lambda: det.read_class_rows(*args, hoff, nrows),
                      fit_c2=fit)
        ms = {r: [] for r in routes}
        out = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out[r] = timed_events(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        f = out['fit_c2']
        per_site = torch.diff(rows['soff'])
        row = dict(shape=name, reads=nreads, events=nreads * read_len, sites=nsites, rows=nrows, rows_per_read=nrows // nreads,
                   rows_per_site_max=int(per_site.max().item()), fit_steps=f['n_iter'], fit_converged=f['converged'], fit_ll=f['ll'],
                   fit_weights=sorted(f['w'].cpu().tolist()), **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            work = nrows * (f['n_iter'] if r == 'fit_c2' else 1)
            row[r]['rows_per_s'] = work / (row[r]['median'] / 1e3)
            row[r]['over_k19_all'] = row[r]['median'] / row['k19_all']['median']
        row['fit_c2']['per_step_over_k19_all'] = row['fit_c2']['over_k19_all'] / f['n_iter']
        note(json.dumps(row))
        out_rows.append(row)
        del out, score, rows
    for row in out_rows:
        print(json.dumps(row))
    if a.write:
        with open(a.write, 'a') as fh:
            fh.writelines(json.dumps(row) + '\n' for row in out_rows)


if __name__ == '__main__':
    main()
