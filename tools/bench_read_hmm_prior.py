#!/usr/bin/env python3
"""Side measurement of the read chain with a per-site prior (K23) on one GPU, not the headline bench: bench_read_hmm.py's sibling.

Per shape, alternated in one loop and timed with HIP events: the plain entries nmod_read_hmm (every output), nmod_read_viterbi (every
output) and nmod_read_hmm_grad (the sums) and, where the tree under --root has them, the same three with site_pi (the shares drawn
uniformly from 0.02 .. 0.98, every twentieth a NaN).  Shapes: bench_read_hmm.py's first wave form and first workgroup form (every tenth
position a candidate site, reads of 2 000 events = 200 entries and of 20 000 events = 2 000 entries).  Reported per route: the median
of `steps` calls after a warm-up, their minimum and maximum, entries/s at the median; per pair the ratio prior / plain of the medians.
The gather kernel of the prior entries (rh_share_kernel) is inside those calls; its own time comes from a kernel trace of this tool
(profiles/read_hmm_prior.txt has the command).

--root DIR imports the package (and its library) of another checkout: the parent commit's, built beside this one, for the plain
entries against the parent; the two are run in turn, at least three pairs, both with --plain-only: what ran before a call moves its
time by more than the run-to-run spread, so the two sides must run the same loop.  One JSON line per shape; --write FILE appends them.

    python tools/bench_read_hmm_prior.py [--root DIR] [--plain-only] [--steps 5] [--warmup 1] [--write FILE]
"""
import argparse
import inspect
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--warmup', type=int, default=1)
ap.add_argument('--write', default='')
ap.add_argument('--plain-only', action='store_true', help='the plain entries alone: the loop the parent commit can run too')
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
import torch
import nanomod_amd as nm

L = nm._lib
_T0 = time.time()
SHAPES = ((2000, 20000), (20000, 2000))


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
    a = ARGS
    if not torch.cuda.is_available():
        sys.exit('bench_read_hmm_prior: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    has_prior = 'site_pi' in inspect.signature(det.read_hmm).parameters and not a.plain_only
    note(os.path.abspath(a.root), L.load().nmod_build_info().decode(), 'prior entries: %s' % has_prior)
    rows = []
    for read_len, nreads in SHAPES:
        g = torch.Generator(dev).manual_seed(19)
        span = 4 * read_len
        start = torch.randint(0, span - read_len + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
        cs = torch.randint(0, 2, (nreads,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
        z = (torch.arange(nreads * read_len, device=dev) // 500) % 3 == 0
        score = 2.0 * (torch.randn(nreads * read_len, device=dev, generator=g, dtype=torch.float64) + 2.0 * z) - 2.0
        pos = torch.arange(span // 10, device=dev, dtype=torch.int64) * 10
        key = torch.cat([pos, (1 << 40) | pos])
        args = (cs, start, roff, score, key)
        (hoff, nrows) = det.read_sites(*args)
        kw = dict(pi=0.33, length=2000.0)
        routes = dict(hmm=lambda: det.read_hmm(*args, hoff, nrows, **kw), viterbi=lambda: det.read_viterbi(*args, hoff, nrows, **kw),
                      grad=lambda: det.read_hmm_grad(*args, hoff, nrows, want=('sums',), **kw))
        if has_prior:
            site_pi = 0.02 + 0.96 * torch.rand(key.numel(), device=dev, generator=g, dtype=torch.float64)
            site_pi[::20] = float('nan')
            routes.update(hmm_prior=lambda: det.read_hmm(*args, hoff, nrows, site_pi=site_pi, **kw),
                          viterbi_prior=lambda: det.read_viterbi(*args, hoff, nrows, site_pi=site_pi, **kw),
                          grad_prior=lambda: det.read_hmm_grad(*args, hoff, nrows, want=('sums',), site_pi=site_pi, **kw))
        ms = {r: [] for r in routes}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, _ = timed_events(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        per_read = nrows // nreads
        row = dict(root=os.path.abspath(a.root), plain_only=bool(a.plain_only), form='wave' if per_read <= L.HMM_WAVE_MAX else 'workgroup', reads=nreads, entries=nrows,
                   entries_per_read=per_read, sites=int(key.numel()), **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            row[r]['entries_per_s'] = nrows / (row[r]['median'] / 1e3)
        if has_prior:
            row['prior_over_plain'] = {r: row[r + '_prior']['median'] / row[r]['median'] for r in ('hmm', 'viterbi', 'grad')}
        note(json.dumps(row))
        rows.append(row)
        del score
    for row in rows:
        print(json.dumps(row))
    if a.write:
        with open(a.write, 'a') as f:
            f.writelines(json.dumps(row) + '\n' for row in rows)


if __name__ == '__main__':
    main()
