#!/usr/bin/env python3
"""Side measurement of nmod_kmer_model (K10) on one GPU, not the headline bench: DeviceDetector.kmer_model on event-like rows of
nmod_synth_fill_events with k = 6 (4 096 codes), int16 and float32, at 4.6 M x 200 and at the configs[4] ragged sizes — and, in the
same process on the same rows, what the tree offered for this reduction before the entry existed: onesample.profile_moments (a K9
run against a dummy reference: a sort and n erfc per position) plus np.bincount pooling on the host.

Each device call is timed by its own pair of HIP events after a warm-up; the figure is the median.  The bytes are what the
algorithm has to read: the samples once, 8 bytes of offsets (CSR) and 4 of code per position.  One JSON line per leg; --write FILE
also writes the record kept as profiles/kmer_model.txt (with the compiler's resource usage of kmer_model.hip).

    python tools/bench_kmer_model.py [--steps 11] [--warmup 3] [--legs 200,ragged] [--scale 1.0] [--write profiles/kmer_model.txt]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nanomod_amd as nm
from nanomod_amd import onesample

L = nm._lib
DEV = 'cuda:0'
K = 6
NCODES = 4 ** K
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12          # bytes / s: the data-sheet rate and the measured copy rate (MI355X_MICROARCH.md)


def timed_median(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def parent_route(sig, off, codes, reps):
    """per-position moments by K9 against a dummy reference (the only way the tree had), pooled per code with np.bincount"""
    times, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        mean, sd, status = onesample.profile_moments(sig, off)
        n = np.diff(off).astype(np.float64)
        ok = (status & (L.STATUS_TOO_LARGE | L.STATUS_NONFINITE | L.STATUS_EMPTY)) == 0
        c, w = codes[ok], n[ok]
        N = np.bincount(c, weights=w, minlength=NCODES)
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.bincount(c, weights=w * mean[ok], minlength=NCODES) / N
            q = np.bincount(c, weights=w * (sd[ok] ** 2 + mean[ok] ** 2), minlength=NCODES) / N
            res = (N, m, np.sqrt(np.maximum(q - m * m, 0.0)))
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), res


def leg(name, npos, n, dtype, steps, warmup, parent_reps, off=None, seed=7):
    det = nm.DeviceDetector(0)
    total = int(off[-1]) if off is not None else npos * n
    doff = torch.from_numpy(off).to(DEV) if off is not None else None
    sig = torch.empty(total, dtype=dtype, device=DEV)
    det.synth_fill_events(sig, seed, 0, npos, 0, n_per_pos=0 if off is not None else n, off=doff)
    codes = torch.randint(0, NCODES, (npos,), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(seed))
    stride = 0 if off is not None else n
    out = det.kmer_model(sig, codes, NCODES, off=doff, stride=stride)
    ms, lo, hi = timed_median(lambda: det.kmer_model(sig, codes, NCODES, off=doff, stride=stride, out=out), steps, warmup)
    nbytes = total * sig.element_size() + (8 * (npos + 1) if off is not None else 0) + 4 * npos
    rate = nbytes / (ms * 1e-3)
    rec = {'leg': name, 'dtype': str(dtype).split('.')[-1], 'k': K, 'positions': npos, 'samples': total, 'bytes': nbytes,
           'bytes_per_position': nbytes / npos, 'kmer_model_ms': ms, 'kmer_model_ms_min': lo, 'kmer_model_ms_max': hi, 'steps': steps,
           'GBps': rate / 1e9, 'of_8TBps': rate / HBM_PEAK, 'of_copy_rate': rate / HBM_COPY}
    if parent_reps:
        h_off = off if off is not None else np.arange(npos + 1, dtype=np.int64) * n
        h_codes = codes.cpu().numpy().astype(np.int64)
        p_ms, (pN, pm, psd) = parent_route(sig.cpu().numpy(), h_off, h_codes, parent_reps)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        seen = got['n_samples'] > 0
        rec.update(parent_route_ms=p_ms, parent_reps=parent_reps, parent_over_kmer_model=p_ms / ms,
                   max_abs_diff_mean=float(np.abs(got['mean'][seen] - pm[seen]).max()), max_abs_diff_sd=float(np.abs(got['sd'][seen] - psd[seen]).max()),
                   counts_equal=bool(np.array_equal(got['n_samples'], pN.astype(np.int64))))
    print(json.dumps(rec), flush=True)
    return rec


def resource_usage():
    """the -Rpass-analysis=kernel-resource-usage lines of kmer_model.hip's own kernels, one line per kernel"""
    src = os.path.join(ROOT, 'nanomod_amd', 'csrc', 'kmer_model.hip')
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-c', src, '-o', os.devnull,
           '-Rpass-analysis=kernel-resource-usage']
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    lines, cur = [], None
    for ln in err.splitlines():
        m = re.search(r'remark: (?:\s*)(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|'
                      r'LDS Size \[bytes/block\]): (\S+)', ln)
        if not m or 'kmer_model.hip' not in ln:
            continue
        if m.group(1) == 'Function Name':
            cur = [m.group(2)]
            lines.append(cur)
        elif cur is not None:
            cur.append('%s: %s' % (m.group(1), m.group(2)))
    return ['  ' + ' '.join(x) for x in lines]


def write_record(path, recs, resource, notes):
    with open(path, 'w') as f:
        f.write('nmod_kmer_model (K10) — resource usage and measurements\n')
        f.write('=======================================================\n\n')
        f.write('1. Resource usage of the built ISA (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage, kmer_model.hip)\n')
        f.write('   km_i16_kernel<LDS_TABLE, CLIP> (mangled: ...ILb<LDS_TABLE>ELb<CLIP>E); km_moments_kernel<DT> (DT 0 = float32, 2 = float64)\n\n')
        f.write('\n'.join(resource) + '\n\n')
        f.write('2. Throughput (tools/bench_kmer_model.py on one MI355X: k = 6, 4 096 codes, no keep bounds; HIP events around each call,\n')
        f.write('   median of `steps` after a warm-up).  bytes = samples + 8 per position of offsets (CSR legs) + 4 per position of code.\n')
        f.write('   parent route = onesample.profile_moments (K9 against a dummy reference, host entry) + np.bincount pooling, host clock.\n\n')
        for r in recs:
            f.write('   %s, %s: %d positions, %d samples, %.1f bytes per position\n' % (r['leg'], r['dtype'], r['positions'], r['samples'], r['bytes_per_position']))
            f.write('     nmod_kmer_model  %.3f ms (min %.3f, max %.3f, %d calls)   %.1f GB/s = %.3f of 8 TB/s = %.3f of the 6.29 TB/s copy rate\n'
                    % (r['kmer_model_ms'], r['kmer_model_ms_min'], r['kmer_model_ms_max'], r['steps'], r['GBps'], r['of_8TBps'], r['of_copy_rate']))
            if 'parent_route_ms' in r:
                f.write('     parent route     %.1f ms (median of %d)   ratio %.0f x   |mean diff| <= %.2e, |sd diff| <= %.2e, counts equal: %s\n'
                        % (r['parent_route_ms'], r['parent_reps'], r['parent_over_kmer_model'], r['max_abs_diff_mean'], r['max_abs_diff_sd'], r['counts_equal']))
        if notes:
            f.write('\n' + open(notes).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--legs', default='200,ragged')
    ap.add_argument('--dtypes', default='int16,float32')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the positions of every leg')
    ap.add_argument('--parent-reps', type=int, default=3, help='repetitions of the parent route (0: leave it out)')
    ap.add_argument('--write', default='', help='write the record (profiles/kmer_model.txt) here')
    ap.add_argument('--resource-file', default='', help='with --write: resource usage lines captured earlier instead of a compile now')
    ap.add_argument('--notes', default='', help='with --write: a text file appended as section 3 (what bounds the kernel, counters)')
    a = ap.parse_args()
    if a.steps < 10:
        ap.error('--steps: the median is of at least 10 calls')
    legs = a.legs.split(',')
    dts = [{'int16': torch.int16, 'float32': torch.float32}[d] for d in a.dtypes.split(',')]
    sc = lambda p: max(int(p * a.scale), 1024)
    recs = []
    if '200' in legs:
        for dt in dts:
            recs.append(leg('4.6M x 200', sc(4_600_000), 200, dt, a.steps, a.warmup, a.parent_reps))
    if 'ragged' in legs:                       # the group-1 sizes of BASELINE.json configs[4]: LogNormal(ln 1000, 0.5) in [5, 4000]
        P = sc(1_000_000)
        n0 = np.clip(np.round(np.random.default_rng(5).lognormal(np.log(1000), 0.5, P)), 5, 4000).astype(np.int64)
        off = np.zeros(P + 1, np.int64); off[1:] = np.cumsum(n0)
        for dt in dts:
            recs.append(leg('configs[4] ragged ~1000', P, 1000, dt, a.steps, a.warmup, a.parent_reps, off=off))
    if a.write:
        resource = open(a.resource_file).read().rstrip('\n').splitlines() if a.resource_file else resource_usage()
        write_record(a.write, recs, resource, a.notes)


if __name__ == '__main__':
    main()
