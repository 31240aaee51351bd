"""Read-level input of `detect` at E. coli scale: nmod_pivot_reads / nmod_select_tested / nmod_gather_tested (read_pivot.hip).

Seeded read sets shaped like an E. coli run: one 4.6 Mb contig, both strands, lognormal read lengths around 8 kb, int16
milli-unit values, two groups, at the given fractions of 200x per strand.  Per group: the host->device copy and the pivot;
per pair: select and gather; each library call timed with HIP events (engine's `timer=`), in events/s.  At --cli-fraction
the wall time of `cli detect` on read-level containers; at --gb-fraction fast5_ingest.GroupBuilder on the host.

    python tools/read_pivot_sweep.py --fractions 0.01,0.1,1.0 --out profiles/read_pivot.txt
"""
import argparse
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENOME = 4_600_000
DEPTH = 200


def make_reads(seed, fraction):
    rng = np.random.default_rng(seed)
    target = int(GENOME * DEPTH * 2 * fraction)              # events over both strands
    lens = []
    total = 0
    while total < target:
        ln = np.clip(rng.lognormal(np.log(8000), 0.5, 65536).astype(np.int64), 200, 60000)
        lens.append(ln); total += int(ln.sum())
    lens = np.concatenate(lens)
    lens = lens[:np.searchsorted(np.cumsum(lens), target) + 1]
    n = len(lens)
    start = (rng.random(n) * (GENOME - lens)).astype(np.int64)
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
    vals = rng.integers(-2500, 2500, off[-1], dtype=np.int16)
    base = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, off[-1], dtype=np.uint8)].view('S1')
    return dict(chrom=np.full(n, 'NC_000913.3'), strand=np.where(rng.random(n) < 0.5, '+', '-'), start=start, off=off,
                norm_mean=vals, base=base)


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); r = fn(); b.record()
    torch.cuda.synchronize()
    return r, a.elapsed_time(b) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fractions', default='0.01,0.1,1.0')
    ap.add_argument('--cli-fraction', type=float, default=0.1)
    ap.add_argument('--gb-fraction', type=float, default=0.01)
    ap.add_argument('--out', default='')
    ap.add_argument('--no-extras', action='store_true', help='only the device legs (for profiler runs)')
    a = ap.parse_args()
    import torch
    import nanomod_amd as nm
    from nanomod_amd import cli, container, engine, fast5_ingest
    L = nm._lib
    lib = L.load()
    so = L.LIB_PATH
    sha = hashlib.sha256(open(so, 'rb').read()).hexdigest()[:16]
    lines = ['# tools/read_pivot_sweep.py  libnanomod_hip.so sha256[:16]=%s  %s' % (sha, torch.cuda.get_device_name(0)),
             '# device time (HIP events around each library call; its few small read-backs of sizes included), seconds',
             '# fraction  group  reads  events  h2d_s  pivot_s  pivot_ev/s  | select_s  gather_s  tested  both groups: (pivot+select+gather)_s  ev/s']
    engine.warm_up(0); engine._join_warm_up(0)
    for f in [float(x) for x in a.fractions.split(',')]:
        groups, ev_total, t_dev = [], 0, 0.0
        for g in (0, 1):
            r = make_reads(100 + g, f)
            nev = int(r['off'][-1]); ev_total += nev
            tm = {}
            groups.append(engine.pivot_reads(r, 0, timer=tm))
            t_dev += tm['pivot']
            lines.append('%8.2f  %5d  %7d  %11d  %6.3f  %7.3f  %10.3e  |' % (f, g, len(r['start']), nev, tm['h2d'], tm['pivot'],
                                                                          nev / max(tm['pivot'], 1e-9)))
            del r
        tm = {}
        res = engine.select_tested(groups[0], groups[1], 5, log=lambda *x: None, timer=tm)
        t_dev += tm['select'] + tm.get('gather', 0.0)
        lines[-1] += '  %7.3f  %7.3f  %8d  %7.3f  %.3e' % (tm['select'], tm.get('gather', 0.0), len(res[0]['pos']), t_dev, ev_total / max(t_dev, 1e-9))
        print('\n'.join(lines[-2:]), flush=True)
        del groups, res
        torch.cuda.empty_cache(); lib.nmod_trim_scratch(0)
    if a.no_extras:
        lines.append('# (--no-extras: no cli / GroupBuilder legs)')
        return finish(lines, a.out)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for g in (0, 1):
            r = make_reads(100 + g, a.cli_fraction)
            paths.append(os.path.join(tmp, 'g%d.npz' % g))
            container.save_reads(paths[-1], r['chrom'], r['strand'], r['start'], r['off'], r['norm_mean'], r['base'])
        t0 = time.time()
        rc = cli.main(['detect', '--wrkBase1', paths[0], '--wrkBase2', paths[1], '--outFolder', os.path.join(tmp, 'o'), '--outLevel', '3',
                       '--SaveTest', '0'])
        lines.append('# cli detect on read-level containers at %.2f: %.2f s wall (rc %d)' % (a.cli_fraction, time.time() - t0, rc))
        r = make_reads(100, a.gb_fraction)
        v = r['norm_mean'].astype(np.float64) / 1000.0
        t0 = time.time()
        gb = fast5_ingest.GroupBuilder({'min_lr': 0}, log=lambda *x: None)
        for i in range(len(r['start'])):
            s, e = r['off'][i], r['off'][i + 1]
            gb.add_read(str(r['chrom'][i]), int(r['start'][i]), str(r['strand'][i]), v[s:e], r['base'][s:e])
        gb.finish()
        dt = time.time() - t0
        lines.append('# GroupBuilder (host) at %.2f: %d events in %.2f s = %.3e events/s' % (a.gb_fraction, int(r['off'][-1]), dt, r['off'][-1] / dt))
    print('\n'.join(lines[-2:]))
    finish(lines, a.out)


def finish(lines, out):
    if out:
        os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
        with open(out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
