"""Deep-coverage sweep (NMOD_FLAG_DEEP): device-resident fixed-stride batches of positions with groups beyond 65 535 samples,
timed with HIP events after a warm-up, float32 continuous rows (nmod_synth_fill) and int16 event-like rows
(nmod_synth_fill_events), all tests and KS-only.  Prints one line per configuration and writes them, with the library's sha,
to --out (profiles/deep_coverage.txt).  --oracle adds the 16-thread C oracle's rate on one position of each shape.
    python tools/deep_coverage_sweep.py [--reps 3] [--oracle] [--out profiles/deep_coverage.txt]"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))

import numpy as np
import torch

import nanomod_amd as nm
from nanomod_amd import _lib as L

SHAPES = [(512, 100000), (64, 1000000), (4, 2000000)]
TARGET = 1e9          # samples / s (the issue's estimate for a merge scheme streaming ~50 B per sample)


def lib_sha():
    with open(os.path.join(ROOT, 'nanomod_amd', 'libnanomod_hip.so'), 'rb') as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def run_one(npos, n, kind, tests, reps):
    dev = 'cuda:0'
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer' if tests == L.TEST_ALL else 'ks', tests=tests, deep=True)
    dt = torch.float32 if kind == 'f32' else torch.int16
    s0 = torch.empty(npos * n, dtype=dt, device=dev); s1 = torch.empty(npos * n, dtype=dt, device=dev)
    if kind == 'f32':
        det.synth_fill(s0, 7, 0, npos, 0, n, 100, 0.01); det.synth_fill(s1, 7, 0, npos, 1, n, 100, 0.01)
    else:
        det.synth_fill_events(s0, 7, 0, npos, 0, n_per_pos=n, plant_period=100, plant_shift_milli=20, spread_milli=200)
        det.synth_fill_events(s1, 7, 0, npos, 1, n_per_pos=n, plant_period=100, plant_shift_milli=20, spread_milli=200)
    rid = torch.zeros(npos, dtype=torch.int32, device=dev)
    out = det.run(s0, s1, rid, stride0=n, stride1=n, npos=npos)        # warm-up (allocations, pool)
    torch.cuda.synchronize()
    st = det.dispatch_stats()
    assert st['deep'] == npos, st
    assert int((out['status'] & L.STATUS_TOO_LARGE).sum().item()) == 0
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        det.run(s0, s1, rid, stride0=n, stride1=n, npos=npos, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del s0, s1
    return float(np.median(ms))


def oracle_rate(n, kind, tests):
    import oracle_c
    rng = np.random.default_rng(1)
    if kind == 'f32':
        a = rng.standard_normal(n).astype(np.float32); b = rng.standard_normal(n).astype(np.float32)
    else:
        a = np.rint(rng.standard_normal(n) * 200).astype(np.int16); b = np.rint(rng.standard_normal(n) * 200).astype(np.int16)
    off = np.array([0, n], np.int64)
    t = time.time()
    oracle_c.detect_batch(a, off, b, off, np.zeros(1, np.int32), 2, 2.0, 'stouffer' if tests == 7 else 'ks', tests=tests, threads=16)
    return 2.0 * n / (time.time() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--oracle', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deep_coverage.txt'))
    a = ap.parse_args()
    lines = ['# deep-coverage sweep (NMOD_FLAG_DEEP), library sha %s, device-resident fixed-stride batches, median of %d '
             'HIP-event-timed runs after a warm-up; target %.0e samples/s' % (lib_sha(), a.reps, TARGET),
             '# npos x n v n      rows  tests   ms        positions/s   samples/s    vs target   C oracle (16 thr) samples/s']
    for npos, n in SHAPES:
        for kind in ('f32', 'i16'):
            for tests in (L.TEST_ALL, L.TEST_KS):
                ms = run_one(npos, n, kind, tests, a.reps)
                sps = 2.0 * npos * n / (ms * 1e-3)
                orc = ('%.3e' % oracle_rate(n, kind, tests)) if a.oracle else '-'
                line = '%4d x %8d v %8d  %s  %-5s  %9.3f  %11.4g  %11.4g  %6.2fx   %s' % (
                    npos, n, n, kind, 'all' if tests == L.TEST_ALL else 'ks', ms, npos / (ms * 1e-3), sps, sps / TARGET, orc)
                print(line, flush=True)
                lines.append(line)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
