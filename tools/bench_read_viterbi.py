#!/usr/bin/env python3
"""Side measurement of the per-read Viterbi decoding of the site chain (K20) on one GPU, not the headline bench.

Per shape: DeviceDetector.read_viterbi (nmod_read_viterbi, HIP events on the stream) for four request sets — `vit` alone (the forward
pass), `path` (forward and traceback), `path` and `delta` (all three passes), every output — and, as the yardstick on the same inputs
in the same loop, DeviceDetector.read_hmm (nmod_read_hmm, K19) with `ll` alone (its forward pass) and with `post` (forward and
backward).  The routes alternate inside one loop, so drift of the clocks meets all of them alike.  Every call fills the entries first
(the same kernel in both entries).  Shapes: every tenth position a candidate site, window sums drawn from two levels 2 sd apart in
stretches (every score valid); reads of 16, 256 and 1 024 entries (the wave form) and of 8 192 entries (the workgroup form), about
four million entries a batch.
Reported: entries/s.  The figure is the median of `steps` calls after a warm-up, the spread their minimum and maximum.  One JSON line
per row; --write FILE appends them.

    python tools/bench_read_viterbi.py [--steps 7] [--warmup 2] [--write FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def spread(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--write', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_viterbi: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    note(L.load().nmod_build_info().decode())
    rows = []
    for per_read, nreads in ((16, 250000), (256, 16000), (1024, 4000), (8192, 500)):
        read_len = 10 * per_read
        g = torch.Generator(dev).manual_seed(20)
        span = 4 * read_len
        start = torch.randint(0, span - read_len + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
        cs = torch.randint(0, 2, (nreads,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
        # stretches of a quarter of a read at the modified level on a third of it
        z = (torch.arange(nreads * read_len, device=dev) // max(read_len // 4, 1)) % 3 == 0
        score = 2.0 * (torch.randn(nreads * read_len, device=dev, generator=g, dtype=torch.float64) + 2.0 * z) - 2.0
        pos = torch.arange(span // 10, device=dev, dtype=torch.int64) * 10
        key = torch.cat([pos, (1 << 40) | pos])
        args = (cs, start, roff, score, key)
        (hoff, nrows) = det.read_sites(*args)
        kw = dict(pi=0.33, length=float(read_len) / 5.0)
        vit = lambda want: (lambda: det.read_viterbi(*args, hoff, nrows, want=want, **kw))
        hmm = lambda want: (lambda: det.read_hmm(*args, hoff, nrows, want=want, **kw))
        routes = dict(vit_only=vit(('vit',)), path=vit(('path',)), path_delta=vit(('path', 'delta')), all=vit(nm.engine.VIT_OUTPUTS),
                      hmm_ll_only=hmm(('ll',)), hmm_post=hmm(('post',)))
        ms = {r: [] for r in routes}
        out = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out[r] = timed_events(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        row = dict(form='wave' if nrows // nreads <= L.HMM_WAVE_MAX else 'workgroup', reads=nreads, events=nreads * read_len, sites=int(key.numel()),
                   entries=nrows, entries_per_read=nrows / nreads, domains=int(out['all']['n_runs'].sum()), **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            row[r]['entries_per_s'] = nrows / (row[r]['median'] / 1e3)
        row['forward_vs_k19'] = row['hmm_ll_only']['median'] / row['vit_only']['median']      # above 1: the (max, +) forward pass is the faster
        note(json.dumps(row))
        rows.append(row)
        del out, score
    for row in rows:
        print(json.dumps(row))
    if a.write:
        with open(a.write, 'a') as f:
            f.writelines(json.dumps(row) + '\n' for row in rows)


if __name__ == '__main__':
    main()
