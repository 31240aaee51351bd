#!/usr/bin/env python3
"""Times nmod_fdr_adjust (K7, nanomod_amd/csrc/fdr.hip) on the device against what the library offered before it.

One process, every shape warmed up, HIP-event times over enough repeats to fill about a second, the routes alternated inside
one loop.  Per size (4.6 M: comb_p of an actual configs[1] step; 80 M: uniform, the gathered track of the eight-GPU ragged
preset) and per method (bh, by):
  new      DeviceDetector.fdr on the device-resident track (one track, summary left on the device)
  pieces   the same q from the entries that existed before: nmod_argsort_keys on the int64 image of the track, then torch
           gather / flip / cummin / flip / scatter on the device
  host     D2H copy + scipy.stats.false_discovery_control on this machine's CPU (a single run)
and the time of one detect step at 4.6 M for scale.  The bytes per element of `new` are computed from its pass structure and
turned into a streaming bound at 8 TB/s: the least time HBM could take to move them, not a claim that the sort is a stream.
Prints one JSON line; writes the table to --out (default profiles/fdr_adjust.txt).  Inputs come from a seed."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12
RS_TILE = 2048


def bytes_per_element(n):
    """HBM traffic of one track through fdr.hip, from its passes: bytes read + written per element"""
    key_pass = 8 + (8 + 4)                                   # p -> key, index
    hist = 256 * 4 / RS_TILE                                  # a tile's histogram row, per element
    sort_pass = 8 + 4 * hist + (8 + 4) + (8 + 4)             # histogram pass reads keys; scan reads/writes hist twice; scatter moves the pairs
    step_up = 8 + (8 + 4) + 8                                 # tile minima read keys; apply reads pairs, writes q (the scatter by index)
    return key_pass + 8 * sort_pass + step_up


def event_time(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sizes', default='4600000,80000000')
    ap.add_argument('--seconds', type=float, default=1.0, help='timed window per route')
    ap.add_argument('--no-baselines', action='store_true', help='time only the new entry (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'fdr_adjust.txt'))
    ap.add_argument('--seed', type=int, default=20240601)
    a = ap.parse_args()
    import torch
    import nanomod_amd as nm
    from nanomod_amd import engine
    L = nm._lib
    if not torch.cuda.is_available():
        sys.exit('bench_fdr: no GPU (there is no CPU fallback and no CPU timing)')
    dev = 'cuda:0'
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS)
    result = {'tool': 'bench_fdr', 'device': torch.cuda.get_device_name(0), 'build': L.load().nmod_build_info().decode(), 'sizes': {}}
    lines = ['nmod_fdr_adjust (K7) on %s' % result['device'], 'build: %s' % result['build'],
             'times: HIP events, median (min) over the repeats of a ~%.1f s window per route, routes alternated in one loop' % a.seconds, '']

    def pieces_route(p, method):
        """what a caller could do before K7 without leaving the GPU"""
        n = p.numel()
        order = engine.argsort_device(p.view(torch.int64))                    # NaN (positive quiet) images sort last
        ps = p[order]
        ok = (ps >= 0) & (ps <= 1)
        m = ok.sum()
        i = torch.arange(1, n + 1, device=dev, dtype=torch.float64)
        adj = ps * (m.to(torch.float64) / i)
        if method == 'by':
            adj = adj * torch.where(i <= m, 1.0 / i, torch.zeros_like(i)).sum()
        adj = torch.where(ok, adj, torch.full_like(adj, float('inf')))
        adj = torch.flip(torch.cummin(torch.flip(adj, (0,)), 0).values, (0,)).clamp_(max=1.0)
        adj = torch.where(ok, adj, torch.full_like(adj, float('nan')))
        q = torch.empty_like(p)
        q[order] = adj
        return q

    for n in [int(s) for s in a.sizes.split(',') if s]:
        entry = {}
        if n == 4600000:
            reads = 200
            sig0 = torch.empty(n * reads, dtype=torch.float32, device=dev); sig1 = torch.empty_like(sig0)
            det.synth_fill(sig0, a.seed, 0, n, 0, reads, 10000, 0.8); det.synth_fill(sig1, a.seed, 0, n, 1, reads, 10000, 0.8)
            rid = torch.zeros(n, dtype=torch.int32, device=dev)
            res = det.run(sig0, sig1, rid, stride0=reads, stride1=reads, npos=n)
            torch.cuda.synchronize()
            ts = [event_time(torch, lambda: det.run(sig0, sig1, rid, stride0=reads, stride1=reads, npos=n, out=res))[0] for _ in range(12)]
            entry['detect_step_ms'] = float(np.median(ts[2:]))
            p = res['comb_p'].clone()
            source = 'comb_p of a configs[1] step (4.6 M x 200 v 200, KS + Stouffer window 5)'
            del sig0, sig1
        else:
            p = torch.rand(n, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(a.seed))
            source = 'uniform'
        entry['source'] = source
        bpe = bytes_per_element(n)
        entry['bytes_per_element'] = bpe
        entry['streaming_bound_ms'] = n * bpe / HBM_BYTES_PER_S * 1e3
        lines += ['n = %d  (%s)' % (n, source)]
        if 'detect_step_ms' in entry:
            lines += ['  one detect step (device side), for scale: %.3f ms' % entry['detect_step_ms']]
        lines += ['  new entry moves %.1f B per element (key pass 20, eight sort passes of %.1f, step-up 28): streaming bound %.3f ms at 8 TB/s'
                  % (bpe, (bpe - 48) / 8, entry['streaming_bound_ms'])]
        q_new = torch.empty_like(p)
        for method in ('bh', 'by'):
            new = lambda: det.fdr({'p': p}, tracks=('p',), method=method, alpha=0.05, out={'p': q_new})
            old = lambda: pieces_route(p, method)
            t_new, _ = event_time(torch, new)                                     # warm-up of both shapes, and the window's size
            routes = [('new', new)]
            if not a.no_baselines:
                t_old, q_old = event_time(torch, old)
                t_old, q_old = event_time(torch, old)
                routes.append(('pieces', old))
            t_new, _ = event_time(torch, new)
            reps = max(5, int(math.ceil(a.seconds * 1e3 / max(t_new, 1e-3))))
            reps = min(reps, 400)
            times = {k: [] for k, _ in routes}
            for r in range(reps):
                for k, fn in routes:
                    if k == 'pieces' and r >= max(5, int(math.ceil(a.seconds * 1e3 / t_old))):
                        continue
                    times[k].append(event_time(torch, fn)[0])
            m = {}
            for k in times:
                m[k + '_ms'] = float(np.median(times[k])); m[k + '_min_ms'] = float(np.min(times[k])); m[k + '_reps'] = len(times[k])
            m['fraction_of_streaming_bound'] = entry['streaming_bound_ms'] / m['new_ms']
            m['effective_TBps'] = n * bpe / (m['new_ms'] * 1e-3) / 1e12
            lines += ['  %s  new    %9.3f ms (min %9.3f, %3d reps)  = %.2f TB/s effective, %.1f %% of the 8 TB/s streaming bound'
                      % (method, m['new_ms'], m['new_min_ms'], m['new_reps'], m['effective_TBps'], 100 * m['fraction_of_streaming_bound'])]
            if not a.no_baselines:
                qn, qo = q_new.cpu().numpy(), pieces_route(p, method).cpu().numpy()
                if method == 'bh':
                    m['pieces_equal'] = bool(np.array_equal(qn, qo, equal_nan=True))
                else:
                    with np.errstate(invalid='ignore', divide='ignore'):
                        m['pieces_equal'] = bool(np.array_equal(np.isnan(qn), np.isnan(qo)) and np.nanmax(np.abs(qn - qo) / qo) <= 1e-14)
                m['pieces_over_new'] = m['pieces_ms'] / m['new_ms']
                t0 = time.perf_counter()
                host = p.cpu().numpy()
                t1 = time.perf_counter()
                from scipy.stats import false_discovery_control
                ok = ~np.isnan(host)
                qh = np.full(n, np.nan); qh[ok] = false_discovery_control(host[ok], method=method)
                t2 = time.perf_counter()
                m['host_d2h_ms'] = (t1 - t0) * 1e3; m['host_scipy_ms'] = (t2 - t1) * 1e3
                m['host_equal'] = bool(np.array_equal(qn, qh, equal_nan=True)) if method == 'bh' else \
                    bool(np.nanmax(np.abs(qn - qh) / np.where(qh > 0, qh, 1.0)) <= 1e-14)
                lines += ['  %s  pieces %9.3f ms (min %9.3f, %3d reps)  = %.2f x the new entry; same q: %s'
                          % (method, m['pieces_ms'], m['pieces_min_ms'], m['pieces_reps'], m['pieces_over_new'], m['pieces_equal']),
                          '  %s  host   %9.1f ms D2H + %9.1f ms scipy (one run); same q: %s'
                          % (method, m['host_d2h_ms'], m['host_scipy_ms'], m['host_equal'])]
            entry[method] = m
        lines += ['']
        result['sizes'][str(n)] = entry
        del p, q_new
        torch.cuda.empty_cache()
        L.load().nmod_trim_scratch(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
