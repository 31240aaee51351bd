#!/usr/bin/env python3
"""Side measurement of nmod_one_sample (K9) on one GPU, not the headline bench: DeviceDetector.one_sample on event-like rows of
nmod_synth_fill_events at the shapes below, and — in the same process, on the same rows against an equally deep control — the
two-sample call with tests = KS | WELCH and Stouffer.  One JSON line per leg.

    python tools/bench_one_sample.py [--steps 5] [--warmup 2] [--legs 200,ragged,2048,16384] [--scale 1.0]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import nanomod_amd as nm

L = nm._lib
DEV = 'cuda:0'


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def reference_of(det, npos, seed):
    """a model reference for the rows of the generator: its own level, spread 0.2, and a control depth for the Welch form"""
    pos = np.arange(npos, dtype=np.int64)[:, None]
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import helpers as H
    lev = (H._mix64(np.uint64(seed) ^ np.uint64(0xA5A5A5A5DEADBEEF), pos, 0, np.zeros((1, 1), np.uint64)) >> np.uint64(40)) % np.uint64(6001)
    mu = torch.from_numpy((lev.astype(np.int64).reshape(-1) - 3000) / 1000.0).to(DEV)
    return mu, torch.full((npos,), 0.2, dtype=torch.float64, device=DEV)


def leg(name, npos, n, dtype, steps, warmup, off=None, two_sample=False, seed=7):
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS | L.TEST_WELCH)
    total = int(off[-1]) if off is not None else npos * n
    doff = torch.from_numpy(off).to(DEV) if off is not None else None
    sig = torch.empty(total, dtype=dtype, device=DEV)
    det.synth_fill_events(sig, seed, 0, npos, 0, n_per_pos=0 if off is not None else n, off=doff, plant_period=100, plant_shift_milli=300)
    mu, sd = reference_of(det, npos, seed)
    ref_n = torch.full((npos,), int(n), dtype=torch.int32, device=DEV)
    rid = torch.zeros(npos, dtype=torch.int32, device=DEV)
    out = det.one_sample(sig, mu, sd, ref_n, rid, off=doff, stride=0 if off is not None else n)
    ms = timed(lambda: det.one_sample(sig, mu, sd, ref_n, rid, off=doff, stride=0 if off is not None else n, out=out), steps, warmup)
    rec = {'leg': name, 'dtype': str(dtype).split('.')[-1], 'positions': npos, 'samples': total, 'one_sample_ms': ms,
           'one_sample_positions_per_s': npos / (ms * 1e-3), 'input_GBps': total * sig.element_size() / (ms * 1e-3) / 1e9}
    if two_sample:
        ctl = torch.empty_like(sig)
        det.synth_fill_events(ctl, seed, 0, npos, 1, n_per_pos=n, plant_period=100, plant_shift_milli=300)
        res = det.run(sig, ctl, rid, stride0=n, stride1=n, npos=npos, max_n0=n, max_n1=n)
        ms2 = timed(lambda: det.run(sig, ctl, rid, stride0=n, stride1=n, npos=npos, max_n0=n, max_n1=n, out=res), steps, warmup)
        rec.update(two_sample_ms=ms2, two_sample_positions_per_s=npos / (ms2 * 1e-3), one_over_two=ms / ms2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--legs', default='200,ragged,2048,16384')
    ap.add_argument('--scale', type=float, default=1.0, help='fraction of the positions of every leg')
    a = ap.parse_args()
    legs = a.legs.split(',')
    sc = lambda p: max(int(p * a.scale), 1024)
    if '200' in legs:
        for dt in (torch.float32, torch.int16):
            leg('4.6M x 200 v control 200', sc(4_600_000), 200, dt, a.steps, a.warmup, two_sample=True)
    if 'ragged' in legs:                       # the group-1 sizes of BASELINE.json configs[4]: LogNormal(ln 1000, 0.5) in [5, 4000]
        P = sc(1_000_000)
        n0 = np.clip(np.round(np.random.default_rng(5).lognormal(np.log(1000), 0.5, P)), 5, 4000).astype(np.int64)
        off = np.zeros(P + 1, np.int64); off[1:] = np.cumsum(n0)
        for dt in (torch.float32, torch.int16):
            leg('configs[4] ragged ~1000', P, 1000, dt, a.steps, a.warmup, off=off)
    if '2048' in legs:
        leg('1M x 2048', sc(1_000_000), 2048, torch.float32, a.steps, a.warmup)
    if '16384' in legs:
        leg('100k x 16384', sc(100_000), 16384, torch.float32, a.steps, a.warmup)


if __name__ == '__main__':
    main()
