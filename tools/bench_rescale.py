#!/usr/bin/env python3
"""Side measurement of nmod_rescale_reads (K11) on one GPU, not the headline bench: DeviceDetector.rescale_reads on int16 reads drawn
from a k-mer model on the device — 200 000 reads x 5 000 events at k = 5 and k = 8 with clip_rounds 0 and 2, and a long-tailed set with
lengths log-uniform over 200 .. 200 000 — and, in the same process on the same reads, the same definition written with torch tensor
operations (codes by index arithmetic, fp64 index_add_ segment sums, a chunk of reads at a time).

The entry is timed alone on the whole set; the torch route (minutes per 10^9 events) runs on the first reads of the set, where the
two routes alternate in one loop.  Each call is timed by its own pair of HIP events after a warm-up; the figure is the median; every
stage is reported on stderr as it ends.  The streaming bound is 5 B per int16 event (2 + 1 read, 2 written).  One JSON line per leg;
--write FILE appends the record kept as profiles/rescale_reads.txt.

    python tools/bench_rescale.py [--steps 3] [--warmup 1] [--reads 200000] [--events 5000] [--tail-reads 20000] [--torch-events 20000000]
                                  [--legs 0,1,2,3,4] [--write profiles/rescale_reads.txt]
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
DEV = 'cuda:0'
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes / s: the data-sheet rate and the measured copy rate (MI355X_MICROARCH.md)
BYTES_PER_EVENT = 5
CHUNK_EVENTS = 50_000_000                     # the torch route works on this many events at a time (fp64 temporaries)
OPTS = dict(weighted=True, clip_sigma=3.0, min_events=50, scale_range=(0.5, 2.0))


def _lut():
    lut = torch.full((256,), -1, dtype=torch.int64, device=DEV)
    lut[torch.tensor([ord(c) for c in 'ACGT'], device=DEV)] = torch.arange(4, device=DEV)
    return lut


def chunks(off_host, max_events=CHUNK_EVENTS):
    """consecutive read ranges [r0, r1) of at most max_events events (a longer read alone)"""
    out, r0, n = [], 0, len(off_host) - 1
    while r0 < n:
        r1 = int(np.searchsorted(off_host, off_host[r0] + max_events, side='right')) - 1
        r1 = min(max(r1, r0 + 1), n)
        out.append((r0, r1))
        r0 = r1
    return out


def codes_of(base, rid, j, n_of, e0, k, center, lut):
    """the code of every event of a chunk (events e0 .. e0 + len(rid)) by index arithmetic; -1 without a full ACGT k-mer in the read"""
    v = lut[base.long()]
    n = n_of[rid]
    code = torch.zeros_like(j)
    ok = torch.ones_like(j, dtype=torch.bool)
    here = torch.arange(len(j), device=DEV)
    for d in range(-center, k - center):
        p = j + d
        inside = (p >= 0) & (p < n)
        vv = torch.where(inside, v[(here + d).clamp(0, len(j) - 1)], torch.full_like(j, -1))
        ok &= vv >= 0
        code = code * 4 + vv.clamp(min=0)
    return torch.where(ok, code, torch.full_like(code, -1))


def torch_route(val, off, base, mean, sd, k, center, clip_rounds, off_host, out_val, weighted=True, clip_sigma=3.0, min_events=50,
                scale_range=(0.5, 2.0)):
    """the definition of include/nanomod_hip.h with torch tensor operations: shift, scale, status per read; out_val gets the events"""
    lut = _lut()
    nreads = len(off_host) - 1
    shift = torch.zeros(nreads, dtype=torch.float64, device=DEV)
    scale = torch.ones(nreads, dtype=torch.float64, device=DEV)
    status = torch.zeros(nreads, dtype=torch.uint8, device=DEV)
    lens = off[1:] - off[:-1]
    for r0, r1 in chunks(off_host):
        e0, e1 = int(off_host[r0]), int(off_host[r1])
        m = r1 - r0
        rid = torch.repeat_interleave(torch.arange(m, device=DEV), lens[r0:r1])
        j = torch.arange(e0, e1, device=DEV) - off[r0:r1][rid]
        x = val[e0:e1].double() / 1000.0
        code = codes_of(base[e0:e1], rid, j, lens[r0:r1], e0, k, center, lut)
        c = code.clamp(min=0)
        mu, s = mean[c], sd[c]
        elig = (code >= 0) & torch.isfinite(mu) & torch.isfinite(s) & (s > 0) & torch.isfinite(x)
        w = torch.where(elig, 1.0 / (s * s) if weighted else torch.ones_like(s), torch.zeros_like(s))
        big = torch.full((m,), 1 << 62, dtype=torch.int64, device=DEV)
        first = big.scatter_reduce(0, rid, torch.where(elig, j, torch.full_like(j, 1 << 62)), 'amin')
        has = first < (1 << 62)
        at = (off[r0:r1] - e0 + torch.where(has, first, torch.zeros_like(first))).clamp(max=max(e1 - e0 - 1, 0))
        mu0, x0 = mu[at][rid], x[at][rid]
        dm, dx = mu - mu0, x - x0
        a = torch.zeros(m, dtype=torch.float64, device=DEV)
        b = torch.ones(m, dtype=torch.float64, device=DEV)
        st = torch.zeros(m, dtype=torch.uint8, device=DEV)
        seg = lambda t: torch.zeros(m, dtype=torch.float64, device=DEV).index_add_(0, rid, t)
        for r in range(clip_rounds + 1):
            keep = elig if r == 0 else elig & ((x - a[rid] - b[rid] * mu).abs() <= clip_sigma * b[rid].abs() * s)
            wk = torch.where(keep, w, torch.zeros_like(w))
            cnt, W, sm, sx = seg(keep.double()), seg(wk), seg(wk * dm), seg(wk * dx)
            smm, smx = seg(wk * dm * dm), seg(wk * dm * dx)
            mb, xb = sm / W, sx / W
            Smm, Smx = smm - sm * mb, smx - sm * xb
            bn = Smx / Smm
            few = (st == 0) & (cnt < min_events)
            deg = (st == 0) & ~few & ~((Smm > 0) & torch.isfinite(bn) & (bn > 0))
            st = torch.where(few, torch.full_like(st, 1), torch.where(deg, torch.full_like(st, 2), st))
            live = st == 0
            b = torch.where(live, bn, b)
            a = torch.where(live, (x[at] + xb) - bn * (mu[at] + mb), a)
        st = torch.where((st == 0) & ~((b >= scale_range[0]) & (b <= scale_range[1])), torch.full_like(st, 4), st)
        a = torch.where(st == 0, a, torch.zeros_like(a))
        b = torch.where(st == 0, b, torch.ones_like(b))
        q = torch.round(1000.0 * ((x - a[rid]) * (1.0 / b)[rid]))
        sat = q.abs() > 32767.0
        out_val[e0:e1] = torch.where((st == 0)[rid], q.clamp(-32767.0, 32767.0).to(torch.int16), val[e0:e1])
        st = st | (torch.zeros(m, dtype=torch.float64, device=DEV).index_add_(0, rid, (sat & (st == 0)[rid]).double()) > 0).to(torch.uint8) * 8
        shift[r0:r1], scale[r0:r1], status[r0:r1] = a, b, st
    return shift, scale, status


def make_reads(off_host, mean, sd, k, center, seed):
    """int16 reads drawn from the model on the device: per read a shift in +-0.3 and a scale in 0.8 .. 1.25; 5 % of the events + 1 unit,
    1 % uniform over +-5"""
    g = torch.Generator(DEV).manual_seed(seed)
    off = torch.from_numpy(off_host).to(DEV)
    lens = off[1:] - off[:-1]
    total, nreads = int(off_host[-1]), len(off_host) - 1
    base = torch.tensor([ord(c) for c in 'ACGT'], dtype=torch.uint8, device=DEV)[torch.randint(0, 4, (total,), device=DEV, generator=g)]
    val = torch.empty(total, dtype=torch.int16, device=DEV)
    a = torch.rand(nreads, dtype=torch.float64, device=DEV, generator=g) * 0.6 - 0.3
    b = torch.rand(nreads, dtype=torch.float64, device=DEV, generator=g) * 0.45 + 0.8
    lut = _lut()
    for r0, r1 in chunks(off_host):
        e0, e1 = int(off_host[r0]), int(off_host[r1])
        rid = torch.repeat_interleave(torch.arange(r1 - r0, device=DEV), lens[r0:r1])
        j = torch.arange(e0, e1, device=DEV) - off[r0:r1][rid]
        code = codes_of(base[e0:e1], rid, j, lens[r0:r1], e0, k, center, lut).clamp(min=0)
        z = torch.randn(e1 - e0, dtype=torch.float64, device=DEV, generator=g)
        x = a[r0:r1][rid] + b[r0:r1][rid] * (mean[code] + sd[code] * z)
        u = torch.rand(e1 - e0, device=DEV, generator=g)
        x = torch.where(u < 0.05, x + 1.0, x)
        x = torch.where(u > 0.99, torch.rand(e1 - e0, dtype=torch.float64, device=DEV, generator=g) * 10.0 - 5.0, x)
        val[e0:e1] = torch.round(x.clamp(-30.0, 30.0) * 1000.0).to(torch.int16)
    return off, val, base


_T0 = time.time()


def note(*what):
    """a progress line on stderr"""
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms_list, events):
    ms = float(np.median(ms_list))
    return {'ms_median': round(ms, 3), 'ms_min_max': [round(min(ms_list), 3), round(max(ms_list), 3)], 'events_per_s': float('%.4g' % (events / (ms * 1e-3)))}


def leg(name, off_host, k, clip_rounds, steps, warmup, torch_events, seed=11):
    """One shape and option set.  The entry is timed alone on the whole read set first; the torch route then runs on the first
    reads of the set (up to torch_events events: its fp64 segment sums are orders of magnitude slower than the entry) and the entry is
    timed on those same reads in the same loop, alternating; the ratio is the one of that common subset."""
    center = k // 2
    g = torch.Generator(DEV).manual_seed(100 + k)
    mean = torch.randn(4 ** k, dtype=torch.float64, device=DEV, generator=g)
    sd = torch.rand(4 ** k, dtype=torch.float64, device=DEV, generator=g) * 0.2 + 0.1
    total, nreads = int(off_host[-1]), len(off_host) - 1
    note(name, 'k', k, 'clip_rounds', clip_rounds, ': drawing', total, 'events')
    off, val, base = make_reads(off_host, mean, sd, k, center, seed)
    torch.cuda.synchronize()
    note('reads drawn; the entry alone on all of them')
    det = nm.DeviceDetector(0)
    out = det.rescale_reads(val, off, base, mean, sd, k, center, clip_rounds=clip_rounds, **OPTS)
    torch.cuda.synchronize()
    note('first call done')
    entry = lambda: det.rescale_reads(val, off, base, mean, sd, k, center, clip_rounds=clip_rounds, out=out, **OPTS)
    t_full = []
    for i in range(warmup + steps):
        ms = timed(entry)
        note('entry, whole set: %.3f ms%s' % (ms, ' (warm-up)' if i < warmup else ''))
        if i >= warmup:
            t_full.append(ms)
    full = summary(t_full, total)
    rate = full['events_per_s']
    lens = np.diff(off_host)
    rec = {'leg': name, 'dtype': 'int16', 'k': k, 'center': center, 'clip_rounds': clip_rounds, 'reads': nreads, 'events': total,
           'read_length_min_median_max': [int(lens.min()), int(np.median(lens)), int(lens.max())], 'entry': full,
           'streaming_bytes_per_s': float('%.4g' % (rate * BYTES_PER_EVENT)),
           'share_of_8TBps': round(rate * BYTES_PER_EVENT / HBM_PEAK, 4), 'share_of_measured_copy_6p29TBps': round(rate * BYTES_PER_EVENT / HBM_COPY, 4),
           'fitted_reads': int((out['status'] & L.RESCALE_FAILED == 0).sum()), 'steps': steps, 'warmup': warmup}
    # the common subset: the first reads, up to torch_events events
    m = max(1, min(nreads, int(np.searchsorted(off_host, torch_events, side='right')) - 1))
    sub_host = off_host[:m + 1]
    ev = int(sub_host[-1])
    s_off, s_val, s_base = off[:m + 1].contiguous(), val[:ev].contiguous(), base[:ev].contiguous()
    s_out = det.rescale_reads(s_val, s_off, s_base, mean, sd, k, center, clip_rounds=clip_rounds, **OPTS)
    ref_val = torch.empty_like(s_val)
    s_entry = lambda: det.rescale_reads(s_val, s_off, s_base, mean, sd, k, center, clip_rounds=clip_rounds, out=s_out, **OPTS)
    ref = lambda: torch_route(s_val, s_off, s_base, mean, sd, k, center, clip_rounds, sub_host, ref_val, **OPTS)
    note('torch route on the first', m, 'reads,', ev, 'events')
    t_entry, t_ref = [], []
    for i in range(warmup + steps):                                            # alternated: both see the same machine state
        e_ms = timed(s_entry)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r_shift, r_scale, r_status = ref()
        b.record()
        b.synchronize()
        note('subset: entry %.3f ms, torch %.3f ms%s' % (e_ms, a.elapsed_time(b), ' (warm-up)' if i < warmup else ''))
        if i >= warmup:
            t_entry.append(e_ms)
            t_ref.append(a.elapsed_time(b))
    # the two routes compute the same thing: the same statuses, the pairs to rounding, the events to one unit at a tie
    rec['subset'] = {'reads': m, 'events': ev, 'entry': summary(t_entry, ev), 'torch': summary(t_ref, ev),
                     'ratio_to_torch': round(float(np.median(t_ref)) / float(np.median(t_entry)), 1),
                     'agreement_with_torch': {'same_status': bool((s_out['status'] == r_status).all()),
                                              'max_rel_scale': float((s_out['scale'] / r_scale - 1.0).abs().max()),
                                              'max_abs_shift': float((s_out['shift'] - r_shift).abs().max()),
                                              'max_units_val': int((s_out['val'].int() - ref_val.int()).abs().max())}}
    return rec


LEGS = (('uniform', 5, 0), ('uniform', 5, 2), ('uniform', 8, 0), ('uniform', 8, 2), ('long_tailed', 5, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reads', type=int, default=200000)
    ap.add_argument('--events', type=int, default=5000)
    ap.add_argument('--tail-reads', type=int, default=20000)
    ap.add_argument('--torch-events', type=int, default=20_000_000, help='the torch route runs on the first reads of a set, up to this many events')
    ap.add_argument('--legs', default='0,1,2,3,4', help='which of the five legs to run (a leg per process bounds each by the caller\'s time limit)')
    ap.add_argument('--write', default='', help='append the records to this file (a header first when it does not exist)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rescale: no GPU; this measurement does not fall back')
    uniform = np.arange(a.reads + 1, dtype=np.int64) * a.events
    rng = np.random.default_rng(5)
    tail = np.zeros(a.tail_reads + 1, np.int64)
    tail[1:] = np.cumsum(np.exp(rng.uniform(np.log(200.0), np.log(200000.0), a.tail_reads)).astype(np.int64))
    for i in (int(t) for t in a.legs.split(',')):
        name, k, rounds = LEGS[i]
        rec = leg(name, uniform if name == 'uniform' else tail, k, rounds, a.steps, a.warmup, a.torch_events)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.write:
            fresh = not os.path.exists(a.write)
            with open(a.write, 'a') as f:
                if fresh:
                    f.write('# nmod_rescale_reads (K11), int16 reads drawn from a k-mer model, one MI355X, %s\n' % L.load().nmod_build_info().decode())
                    f.write('# tools/bench_rescale.py: HIP events around each call, medians of `steps` calls after `warmup`.  "entry": the device entry alone on\n'
                            '# the whole read set.  "subset": the same definition in torch tensor operations on the first reads of the set, and the entry on\n'
                            '# those same reads, alternated in one loop; ratio_to_torch is the ratio of that subset.\n')
                    f.write('# streaming bound: %d B per int16 event (2 + 1 read, 2 written); shares are the whole-set entry rate x 5 B over 8 TB/s and 6.29 TB/s\n'
                            % BYTES_PER_EVENT)
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
