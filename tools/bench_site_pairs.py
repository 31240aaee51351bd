#!/usr/bin/env python3
"""Side measurement of nmod_site_pairs (K16) on one GPU, not the headline bench.

--part read: DeviceDetector.site_pairs asked for the counts alone (the read kernel and the zeroing of the counters), as the call picks
  its form ('auto': the LDS table up to NMOD_PAIRS_LDS_MAX pairs, else the counters in device memory), with the direct form forced
  ('direct'), and the same definition in torch tensor operations ('torch': two searchsorted for the sites a read covers, the (read,
  site) and (read, site, partner) lists expanded with repeat_interleave, the calls gathered, index_add_ into the counters), alternated
  in one loop so that all see the same machine state.  Shapes: coverage 30 over 10^4 sites; coverage 1 000 over 10^3 sites; amplicons,
  10^5 reads that each cover all of 40, 100 and 200 sites of their strand (690, 1 890 and 3 890 pairs over both strands: two in the
  table form's range, one beyond it).  Sites lie 10 apart,
  max_dist is 100 (10 partners), a read has a call at a site with probability 0.8.  Reported: reads/s and pair updates/s (the sum of
  the counters) per route, and that the three routes' counters are equal.
--part pair: the pair kernels alone, as the difference between a call that asks for every output and one that asks for the counts, over
  disjoint pairs of sites whose tables have a support of about 51, 251 and 1 001 tables.  Run it under builds of the library with
  another NMOD_PAIRS_THREAD_MAX (NMOD_HIP_LIB) to compare the one-thread and the one-wave form at one support.  The difference of two
  calls of 46 ms carries their noise; for the kernels' own times run one shape (--reads-per-pair) under
  `rocprofv3 --kernel-trace --stats -- python tools/bench_site_pairs.py --part pair --reads-per-pair N` and read sp_pair_kernel and
  sp_pair_wave_kernel off the statistics.

Each call is timed by its own pair of HIP events after a warm-up; the figure is the median of `steps` calls, the spread their minimum
and maximum.  One JSON line per row; --write FILE appends them.

    python tools/bench_site_pairs.py --part read|pair [--steps 5] [--warmup 1] [--write FILE] [--no-torch] [--reads-per-pair N]
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
THR = 2.5


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def make_reads(nreads, read_len, span, nsites, step, seed, dev, p_call=0.8):
    """reads of read_len events with starts spread over [0, span - read_len], both strands of one chromosome; sites every `step`
    positions on both strands; an event is MOD, CAN or none with probabilities p_call / 2, p_call / 2, 1 - p_call"""
    g = torch.Generator(dev).manual_seed(seed)
    start = torch.randint(0, max(span - read_len, 0) + 1, (nreads,), device=dev, generator=g, dtype=torch.int64)
    cs = torch.randint(0, 2, (nreads,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
    roff = torch.arange(nreads + 1, device=dev, dtype=torch.int64) * read_len
    u = torch.rand(nreads * read_len, device=dev, generator=g, dtype=torch.float64)
    score = torch.where(u < p_call / 2, 3.0, torch.where(u < p_call, -3.0, 0.0)).to(torch.float64)
    pos = torch.arange(nsites, device=dev, dtype=torch.int64) * step
    key = torch.cat([pos, (1 << 40) | pos])
    return dict(cs=cs, start=start, roff=roff, score=score, key=key)


def torch_counts(t, poff, npairs):
    """the counts of include/nanomod_hip.h's definition in tensor operations"""
    cs, start, roff, score, key = (t[f] for f in ('cs', 'start', 'roff', 'score', 'key'))
    n = roff[1:] - roff[:-1]
    base = cs.to(torch.int64) << 40
    c_lo = torch.searchsorted(key, base | start)
    c_hi = torch.searchsorted(key, base | (start + n - 1), right=True)
    m = c_hi - c_lo
    read = torch.repeat_interleave(torch.arange(len(cs), device=cs.device), m)          # one entry per (read, covered site)
    site = c_lo[read] + (torch.arange(len(read), device=cs.device) - (torch.cumsum(m, 0) - m)[read])
    pos = key[site] & ((1 << 40) - 1)
    ev = torch.where((cs[read] & 1) != 0, start[read] + n[read] - 1 - pos, pos - start[read])
    s = score[roff[read] + ev]
    call = torch.where(s >= THR, 1, torch.where(s <= -THR, 0, 2))
    reach = torch.minimum(site + 1 + (poff[site + 1] - poff[site]), c_hi[read])
    k = reach - (site + 1)
    keep = call != 2
    ent = torch.repeat_interleave(torch.arange(len(site), device=cs.device)[keep], k[keep])   # one entry per (read, site, partner)
    first = torch.cumsum(k[keep], 0) - k[keep]
    d = torch.arange(len(ent), device=cs.device) - torch.repeat_interleave(first, k[keep])
    cb = call[ent + 1 + d]                                                             # the partner is d + 1 entries on in the read's list
    ok = cb != 2
    cell = 4 * (poff[site[ent]] + d) + 2 * call[ent] + cb
    counts = torch.zeros(4 * npairs, dtype=torch.int32, device=cs.device)
    counts.index_add_(0, cell[ok], torch.ones(int(ok.sum()), dtype=torch.int32, device=cs.device))
    return counts


def part_read(a, det, dev):
    shapes = (('coverage 30, 10^4 sites', 3000, 1000, 100000, 10000), ('coverage 1000, 10^3 sites', 10000, 1000, 10000, 1000),
              ('amplicon, 40 sites', 100000, 400, 400, 40), ('amplicon, 100 sites', 100000, 1000, 1000, 100),
              ('amplicon, 200 sites', 100000, 2000, 2000, 200))
    rows = []
    for name, nreads, read_len, span, nsites in shapes:
        t = make_reads(nreads, read_len, span, nsites, 10, 7, dev)
        poff, npairs = det.pair_index(t['key'], 100)
        args = (t['cs'], t['start'], t['roff'], t['score'], t['key'], poff, npairs)
        routes = dict(auto=lambda: det.site_pairs(*args, thr=THR, want=('counts',))['counts'],
                      direct=lambda: det.site_pairs(*args, thr=THR, want=('counts',), force_direct=True)['counts'])
        if not a.no_torch:
            routes['torch'] = lambda: torch_counts(t, poff, npairs)
        ms = {r: [] for r in routes}
        outs = {}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, outs[r] = timed(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        updates = int(outs['auto'].sum())
        row = dict(part='read', shape=name, reads=nreads, events=nreads * read_len, sites=2 * nsites, pairs=npairs, updates=updates,
                   form='table' if npairs <= L.PAIRS_LDS_MAX else 'direct', equal=all(torch.equal(outs['auto'], o) for o in outs.values()),
                   **{r: spread(v) for r, v in ms.items()})
        for r in routes:
            row[r]['reads_per_s'] = nreads / (row[r]['median'] / 1e3)
            row[r]['updates_per_s'] = updates / (row[r]['median'] / 1e3)
        note(json.dumps(row))
        rows.append(row)
        del t, outs
    return rows


def part_pair(a, det, dev):
    rows = []
    for reads_per_pair, npairs in ((100, 40000), (500, 8000), (2000, 2000)):
        if a.reads_per_pair and reads_per_pair != a.reads_per_pair:
            continue
        g = torch.Generator(dev).manual_seed(11)
        nreads = reads_per_pair * npairs
        pair = torch.arange(nreads, device=dev, dtype=torch.int64) // reads_per_pair
        t = dict(cs=torch.zeros(nreads, dtype=torch.int32, device=dev), start=10 * pair, roff=2 * torch.arange(nreads + 1, device=dev, dtype=torch.int64),
                 score=torch.where(torch.rand(2 * nreads, device=dev, generator=g, dtype=torch.float64) < 0.5, 3.0, -3.0).to(torch.float64),
                 key=(10 * torch.arange(npairs, device=dev, dtype=torch.int64)[:, None] + torch.arange(2, device=dev)[None, :]).reshape(-1))
        poff, n = det.pair_index(t['key'], 1)
        assert n == npairs
        args = (t['cs'], t['start'], t['roff'], t['score'], t['key'], poff, npairs)
        routes = dict(counts=lambda: det.site_pairs(*args, thr=THR, want=('counts',)), all=lambda: det.site_pairs(*args, thr=THR))
        ms = {r: [] for r in routes}
        for step in range(a.warmup + a.steps):
            for r, fn in routes.items():
                dt, out = timed(fn)
                if step >= a.warmup:
                    ms[r].append(dt)
        c = out['counts'].reshape(-1, 4).to(torch.int64)
        support = torch.minimum(c[:, 3] + c[:, 2], c[:, 3] + c[:, 1]) - torch.clamp(c[:, 3] - c[:, 0], min=0) + 1
        row = dict(part='pair', lib=os.path.basename(os.path.dirname(L.LIB_PATH)) + '/' + os.path.basename(L.LIB_PATH), pairs=npairs,
                   reads_per_pair=reads_per_pair, support_median=int(support.median()), support_max=int(support.max()),
                   p_checksum=float(out['p_fisher'].log().sum()), **{r: spread(v) for r, v in ms.items()})
        row['pair_kernels_ms'] = row['all']['median'] - row['counts']['median']
        row['pairs_per_s'] = npairs / (row['pair_kernels_ms'] / 1e3) if row['pair_kernels_ms'] > 0 else None
        note(json.dumps(row))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', choices=['read', 'pair'], required=True)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--reads-per-pair', type=int, default=0, help='--part pair: only this shape (100, 500 or 2000): for a kernel trace of one support')
    ap.add_argument('--write', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_site_pairs: no GPU; nothing is measured without one')
    dev = torch.device('cuda', 0)
    det = nm.DeviceDetector(0)
    note(L.load().nmod_build_info().decode())
    rows = part_read(a, det, dev) if a.part == 'read' else part_pair(a, det, dev)
    for row in rows:
        print(json.dumps(row))
    if a.write:
        with open(a.write, 'a') as f:
            f.writelines(json.dumps(row) + '\n' for row in rows)


if __name__ == '__main__':
    main()
