#!/usr/bin/env python3
"""Side measurement of nmod_read_calls (K12) on one GPU, not the headline bench: DeviceDetector.read_calls on int16 reads drawn from a
k-mer model on the device, and, in the same process on the first reads of the set, the same definition written with torch tensor
operations (codes by index arithmetic, torch.special.erfc / erfcx / gammaincc, the window as 2 nb + 1 shifted masked adds).

Each call is timed by its own pair of HIP events after a warm-up; the figure is the median of `steps` calls (one by default).  The
streaming bound is 3 B read per int16 event (2 + 1) and 8 B written per requested track: 11 B for p_win alone, 27 B for z, p and
p_win.  One JSON line per leg; --write FILE appends the record kept in profiles/read_calls.txt.

    python tools/bench_read_calls.py [--steps 1] [--warmup 1] [--reads 4000] [--events 5000] [--kmer 5] [--nb 2] [--torch-events 2000000]
                                     [--write FILE]
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
DBL_MIN = 2.2250738585072014e-308
INV_SQRT2 = 0.70710678118654752
_T0 = time.time()


def note(*what):
    print('[%7.1f s]' % (time.time() - _T0), *what, file=sys.stderr, flush=True)


def codes_of(base, j, n, k, center):
    """the code of every event (j: its index in its read, n: its read's length) by index arithmetic; -1 without a full ACGT k-mer"""
    lut = torch.full((256,), -1, dtype=torch.int64, device=DEV)
    lut[torch.tensor([ord(c) for c in 'ACGT'], device=DEV)] = torch.arange(4, device=DEV)
    v = lut[base.long()]
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


def torch_route(val, off, base, mean, sd, k, center, nb, alpha):
    """the definition of include/nanomod_hip.h with torch tensor operations: z, p, p_win per event, n_sites, n_called per read"""
    lens = off[1:] - off[:-1]
    m = len(lens)
    rid = torch.repeat_interleave(torch.arange(m, device=DEV), lens)
    j = torch.arange(len(val), device=DEV) - off[:-1][rid]
    n = lens[rid]
    x = val.double() / 1000.0
    code = codes_of(base, j, n, k, center)
    c = code.clamp(min=0)
    mu, s = mean[c], sd[c]
    elig = (code >= 0) & torch.isfinite(mu) & torch.isfinite(s) & (s > 0) & torch.isfinite(x)
    nan = torch.full_like(x, float('nan'))
    z = torch.where(elig, (x - mu) / s, nan)
    u = z.abs() * INV_SQRT2
    p = torch.where(elig, torch.special.erfc(u).clamp(min=DBL_MIN), nan)
    l = torch.where(elig, torch.log(torch.special.erfcx(u)) - u * u, torch.zeros_like(x))
    if nb == 0:
        P = p
    else:
        W = torch.zeros_like(j)
        S = torch.zeros_like(x)
        N = len(x)
        for d in range(-nb, nb + 1):
            src = (torch.arange(N, device=DEV) + d).clamp(0, N - 1)
            part = elig[src] & (j + d >= 0) & (j + d < n)
            W += part
            S = S + torch.where(part, l[src], torch.zeros_like(x))
        P = torch.where(elig, torch.special.gammaincc(W.clamp(min=1).double(), (-S).clamp(min=0)).clamp(min=DBL_MIN), nan)
    seg = lambda t: torch.zeros(m, dtype=torch.int64, device=DEV).index_add_(0, rid, t.long())
    return z, p, P, seg(elig), seg(elig & (P <= alpha))


def make_reads(off_host, mean, sd, k, center, seed):
    """int16 reads drawn from the model on the device; 5 % of the events + 1 unit, 1 % uniform over +-5"""
    g = torch.Generator(DEV).manual_seed(seed)
    off = torch.from_numpy(off_host).to(DEV)
    lens = off[1:] - off[:-1]
    total = int(off_host[-1])
    base = torch.tensor([ord(c) for c in 'ACGT'], dtype=torch.uint8, device=DEV)[torch.randint(0, 4, (total,), device=DEV, generator=g)]
    rid = torch.repeat_interleave(torch.arange(len(lens), device=DEV), lens)
    j = torch.arange(total, device=DEV) - off[:-1][rid]
    code = codes_of(base, j, lens[rid], k, center).clamp(min=0)
    x = mean[code] + sd[code] * torch.randn(total, dtype=torch.float64, device=DEV, generator=g)
    u = torch.rand(total, device=DEV, generator=g)
    x = torch.where(u < 0.05, x + 1.0, x)
    x = torch.where(u > 0.99, torch.rand(total, dtype=torch.float64, device=DEV, generator=g) * 10.0 - 5.0, x)
    return off, torch.round(x.clamp(-30.0, 30.0) * 1000.0).to(torch.int16), base


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def summary(ms_list, events):
    ms = float(np.median(ms_list))
    return {'ms_median': round(ms, 3), 'ms_min_max': [round(min(ms_list), 3), round(max(ms_list), 3)], 'events_per_s': float('%.4g' % (events / (ms * 1e-3)))}


def run(a):
    k, center, nb, alpha = a.kmer, a.kmer // 2, a.nb, 0.01
    g = torch.Generator(DEV).manual_seed(100 + k)
    mean = torch.randn(4 ** k, dtype=torch.float64, device=DEV, generator=g)
    sd = torch.rand(4 ** k, dtype=torch.float64, device=DEV, generator=g) * 0.2 + 0.1
    off_host = np.arange(a.reads + 1, dtype=np.int64) * a.events
    total = int(off_host[-1])
    note('drawing', total, 'events')
    off, val, base = make_reads(off_host, mean, sd, k, center, 11)
    torch.cuda.synchronize()
    det = nm.DeviceDetector(0)
    rec = {'dtype': 'int16', 'k': k, 'center': center, 'nb': nb, 'alpha': alpha, 'reads': a.reads, 'events': total, 'steps': a.steps, 'warmup': a.warmup}
    for want, nbytes in ((('p_win',), 11), (L.CALLS_EVENT_FIELDS, 27)):
        out = det.read_calls(val, off, base, mean, sd, k, center, nb=nb, alpha=alpha, want=want)
        torch.cuda.synchronize()
        ms = []
        for i in range(a.warmup + a.steps):
            t, _ = timed(lambda: det.read_calls(val, off, base, mean, sd, k, center, nb=nb, alpha=alpha, want=want, out=out))
            note('entry, want=%s: %.3f ms%s' % ('+'.join(want), t, ' (warm-up)' if i < a.warmup else ''))
            if i >= a.warmup:
                ms.append(t)
        s = summary(ms, total)
        s.update(streaming_bytes_per_event=nbytes, share_of_8TBps=round(s['events_per_s'] * nbytes / HBM_PEAK, 5),
                 share_of_measured_copy_6p29TBps=round(s['events_per_s'] * nbytes / HBM_COPY, 5))
        rec['entry_' + '_'.join(want)] = s
    rec['called_events'] = int(out['n_called'].sum())
    rec['scored_events'] = int(out['n_sites'].sum())
    # the common subset: the first reads, up to torch_events events
    m = max(1, min(a.reads, a.torch_events // a.events))
    ev = m * a.events
    s_off, s_val, s_base = off[:m + 1].contiguous(), val[:ev].contiguous(), base[:ev].contiguous()
    s_out = det.read_calls(s_val, s_off, s_base, mean, sd, k, center, nb=nb, alpha=alpha)
    t_entry, t_ref = [], []
    for i in range(a.warmup + a.steps):                                        # alternated: both see the same machine state
        e_ms, _ = timed(lambda: det.read_calls(s_val, s_off, s_base, mean, sd, k, center, nb=nb, alpha=alpha, out=s_out))
        r_ms, ref = timed(lambda: torch_route(s_val, s_off, s_base, mean, sd, k, center, nb, alpha))
        note('subset of %d events: entry %.3f ms, torch %.3f ms%s' % (ev, e_ms, r_ms, ' (warm-up)' if i < a.warmup else ''))
        if i >= a.warmup:
            t_entry.append(e_ms)
            t_ref.append(r_ms)
    z, p, P, n_sites, n_called = ref
    ok = ~torch.isnan(P)
    rel = lambda got, exp: float(((got[ok] / exp[ok] - 1.0).abs() * (exp[ok] > DBL_MIN)).max())
    rec['subset'] = {'reads': m, 'events': ev, 'entry': summary(t_entry, ev), 'torch': summary(t_ref, ev),
                     'ratio_to_torch': round(float(np.median(t_ref)) / float(np.median(t_entry)), 1),
                     'agreement_with_torch': {'same_nan_pattern': bool((torch.isnan(s_out['p_win']) == ~ok).all()),
                                              'z_bit_equal': bool((s_out['z'][ok] == z[ok]).all()), 'max_abs_z': float((s_out['z'][ok] - z[ok]).abs().max()),
                                              'max_rel_p': rel(s_out['p'], p), 'max_rel_p_win': rel(s_out['p_win'], P),
                                              'same_n_sites': bool((s_out['n_sites'] == n_sites).all()),
                                              'reads_with_other_n_called': int((s_out['n_called'] != n_called).sum())}}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--events', type=int, default=5000)
    ap.add_argument('--kmer', type=int, default=5)
    ap.add_argument('--nb', type=int, default=2)
    ap.add_argument('--torch-events', type=int, default=2_000_000, help='the torch route runs on the first reads of the set, up to this many events')
    ap.add_argument('--write', default='', help='append the record to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_read_calls: no GPU; this measurement does not fall back')
    rec = run(a)
    rec['build'] = L.load().nmod_build_info().decode()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.write:
        with open(a.write, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
