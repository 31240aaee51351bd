#!/usr/bin/env python3
"""Side measurement of one evaluation of the read chain's likelihood and gradient (K21) on one GPU, not the headline bench.

Per shape: DeviceDetector.read_hmm_grad (nmod_read_hmm_grad: forward pass, backward pass with the gradient terms, the batch sums) with
every output and with `sums` alone (what readllr.fit_hmm asks for per evaluation), alternated IN THE SAME LOOP with
DeviceDetector.read_hmm with every output and with `ll` alone (K19: the full forward-backward call and the forward pass only), so that
the comparison is against K19 on the same run, the same data and the same clocks.  HIP events around every call.  Shapes:
tools/bench_read_hmm.py's four: every tenth position a candidate site, window sums drawn from two levels 2 sd apart in stretches;
  wave form       reads of 2 000 events (200 entries) and of 10 000 events (1 000 entries),
  workgroup form  reads of 20 000 events (2 000 entries) and of 100 000 events (10 000 entries).
Reported: entries/s and the ratio to K19's "all" route.  The figure is the median of `steps` calls after a warm-up, the spread their
minimum and maximum.  One JSON line per row; --write FILE appends them.

    python tools/bench_read_hmm_fit.py [--steps 5] [--warmup 1] [--write FILE]
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
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--write', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_hmm_fit: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    note(L.load().nmod_build_info().decode())
    rows = []
    for read_len, nreads in ((2000, 20000), (10000, 4000), (20000, 2000), (100000, 400)):
        g = torch.Generator(dev).manual_seed(19)
        span = 4 * read_len
        start = torch.randint(0, span - read_len + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
        cs = torch.randint(0, 2, (nreads,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
        # stretches of 500 events at the modified level on a third of the read
        z = (torch.arange(nreads * read_len, device=dev) // 500) % 3 == 0
        score = 2.0 * (torch.randn(nreads * read_len, device=dev, generator=g, dtype=torch.float64) + 2.0 * z) - 2.0
        pos = torch.arange(span // 10, device=dev, dtype=torch.int64) * 10
        key = torch.cat([pos, (1 << 40) | pos])
        args = (cs, start, roff, score, key)
        (hoff, nrows) = det.read_sites(*args)
        kw = dict(pi=0.33, length=2000.0)
        routes = dict(k19_all=lambda: det.read_hmm(*args, hoff, nrows, **kw),
                      k19_ll_only=lambda: det.read_hmm(*args, hoff, nrows, want=('ll',), **kw),
                      grad_all=lambda: det.read_hmm_grad(*args, hoff, nrows, **kw),
                      grad_sums_only=lambda: det.read_hmm_grad(*args, hoff, nrows, want=('sums',), **kw))
        ms = {r: [] for r in routes}
        out = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out[r] = timed_events(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        per_read = nrows // nreads
        sums = out['grad_all']['sums'].cpu().tolist()
        row = dict(form='wave' if per_read <= L.HMM_WAVE_MAX else 'workgroup', reads=nreads, events=nreads * read_len, sites=int(key.numel()),
                   entries=nrows, entries_per_read=per_read, sum_ll=sums[0], sum_g_eta=sums[1], sum_g_lam=sums[2],
                   ll_is_k19s=bool(torch.equal(out['grad_all']['ll'], out['k19_all']['ll'])), **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            row[r]['entries_per_s'] = nrows / (row[r]['median'] / 1e3)
            row[r]['over_k19_all'] = row[r]['median'] / row['k19_all']['median']
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
