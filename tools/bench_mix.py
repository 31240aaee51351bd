#!/usr/bin/env python3
"""Times nmod_mix_fraction (K8, nanomod_amd/csrc/mix_fraction.hip) on the device against what a user of the library could do
before it: the same EM written with torch tensor operations on the device.

One process, every shape warmed up, HIP-event times, the routes alternated inside one loop.  Inputs are event-like int16 rows
(nmod_synth_fill_events: a level per position, spread 0.2, the 3-decimal grid) with group 2 of the planted positions (0, 1, 99
mod 100: 3 %) shifted by 0.8 = 4 sigma.  Configurations:
  ungated   --npos (4.6 M) x 200 v 200, every position computed
  gated     the same rows, gate = the BH q-values of the combined track of a detect step, gate_max = 0.05: the share FDR rejects
  ragged    --ragged-npos positions of 20 .. 400 reads per group (CSR), ungated
Routes:
  new       DeviceDetector.mix (equal-variance model, max_iter 200, tol 1e-6, no per-read output)
  torch     the same iteration on the gated rows, padded to the batch maximum, in chunks of --torch-chunk positions: the parameters of a
            converged position are frozen by a mask, and the loop asks the device every eight iterations whether any position
            is still running.  Checked against `new` on pi / mu_mod / iters before it is timed
Reported per configuration: positions/s, EM exp evaluations/s (sum over computed positions of |Y| x iterations, from the `iters`
output), the ratio to the torch route, and the share of an fp64-issue bound: the iteration loop of mix_em_kernel<16> is 726 fp64
VALU instructions per 16 samples in this build's ISA (45.4 per sample and iteration, the exp's 20-odd among them), and the
MI355X issues 39.3e12 fp64 lane-instructions per second at its 78.6 TFLOP/s vector peak (an FMA counting two), so no form of
this loop can pass 8.7e11 sample-iterations per second.
Prints one JSON line; writes the table to --out (default profiles/mix_fraction.txt).  Inputs come from a seed."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_LANE_INSTR_PER_S = 78.6e12 / 2.0
FP64_INSTR_PER_SAMPLE_ITER = 726.0 / 16.0
ISSUE_BOUND = FP64_LANE_INSTR_PER_S / FP64_INSTR_PER_SAMPLE_ITER


def event_time(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); out = fn(); b.record(); b.synchronize()
    return a.elapsed_time(b), out


def torch_em_chunk(torch, x, nx, y, ny, max_iter, tol):
    """x [P, wx], y [P, wy] float64 rows padded to the chunk's widths, nx / ny [P] valid counts: equal-variance EM of every row"""
    xmask = torch.arange(x.shape[1], device=x.device)[None, :] < nx[:, None]
    mask = torch.arange(y.shape[1], device=y.device)[None, :] < ny[:, None]
    n = ny.to(torch.float64)
    mu = (x * xmask).sum(1) / nx
    s2 = (((x - mu[:, None]) ** 2) * xmask).sum(1) / nx
    s = s2.sqrt()
    d = (y * mask).sum(1) / n - mu
    pi = torch.full_like(mu, 0.5); m = mu + 2.0 * d
    active = torch.ones_like(ny, dtype=torch.bool)
    iters = torch.zeros_like(ny)
    b = (y - mu[:, None]) ** 2 / (2.0 * s2)[:, None]
    for k in range(1, max_iter + 1):
        t = torch.log((1.0 - pi) / pi)[:, None] + (y - m[:, None]) ** 2 / (2.0 * s2)[:, None] - b
        r = mask / (1.0 + torch.exp(t))
        w = r.sum(1)
        pn = w / n; mn = (r * y).sum(1) / w
        delta = torch.maximum((pn - pi).abs(), (mn - m).abs() / s)
        pi = torch.where(active, pn, pi); m = torch.where(active, mn, m)
        iters = iters + active
        active = active & ~(delta <= tol)
        if k % 8 == 0 and not bool(active.any()):
            break
    return pi, m, iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--npos', type=int, default=4600000)
    ap.add_argument('--ragged-npos', type=int, default=1000000)
    ap.add_argument('--reads', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--torch-chunk', type=int, default=131072)
    ap.add_argument('--torch-positions', type=int, default=0, help='time the torch route on the first N positions only (0 = all) and scale')
    ap.add_argument('--no-baselines', action='store_true', help='time only the new entry (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'mix_fraction.txt'))
    ap.add_argument('--seed', type=int, default=20240601)
    a = ap.parse_args()
    import torch
    import nanomod_amd as nm
    L = nm._lib
    if not torch.cuda.is_available():
        sys.exit('bench_mix: no GPU (there is no CPU fallback and no CPU timing)')
    dev = 'cuda:0'
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_KS)
    result = {'tool': 'bench_mix', 'device': torch.cuda.get_device_name(0), 'build': L.load().nmod_build_info().decode(),
              'issue_bound_sample_iters_per_s': ISSUE_BOUND, 'configs': {}}
    lines = ['nmod_mix_fraction (K8) on %s' % result['device'], 'build: %s' % result['build'],
             'times: HIP events, median (min) over %d repeats, routes alternated in one loop; equal-variance model, max_iter 200, tol 1e-6' % a.reps,
             'fp64-issue bound: %.3g sample-iterations/s (45.4 fp64 VALU instructions per sample and iteration at 39.3e12 lane-instructions/s)' % ISSUE_BOUND,
             '']

    def measure(name, what, npos, sig0, sig1, off0, off1, stride, gate):
        kw = dict(off0=off0, off1=off1, stride0=stride, stride1=stride, npos=npos, gate=gate, gate_max=0.05)
        out = det.mix(sig0, sig1, **kw)
        new = lambda: det.mix(sig0, sig1, out=out, **kw)
        event_time(torch, new)
        ny = (off1[1:] - off1[:-1]) if off1 is not None else torch.full((npos,), stride, dtype=torch.int64, device=dev)
        nx = (off0[1:] - off0[:-1]) if off0 is not None else ny
        on = torch.ones(npos, dtype=torch.bool, device=dev) if gate is None else (gate <= 0.05)
        tp = npos if not a.torch_positions else min(npos, a.torch_positions)

        def old():
            rows = on[:tp].nonzero().flatten()               # the gate first: only the rows it lets through are gathered
            pi = torch.full((tp,), float('nan'), dtype=torch.float64, device=dev); mu = pi.clone()
            it = torch.zeros(tp, dtype=torch.int64, device=dev)
            for c0 in range(0, rows.numel(), a.torch_chunk):
                sel = rows[c0:c0 + a.torch_chunk]
                if off1 is None:
                    x = sig0.view(npos, stride)[sel].double() / 1000.0
                    y = sig1.view(npos, stride)[sel].double() / 1000.0
                else:                                        # rows padded to the chunk's maximum
                    def pad(sig, off, cnt):
                        idx = off[sel, None] + torch.arange(int(cnt[sel].max()), device=dev)[None, :]
                        return sig[idx.clamp_(max=sig.numel() - 1)].double() / 1000.0
                    x, y = pad(sig0, off0, nx), pad(sig1, off1, ny)
                pi[sel], mu[sel], it[sel] = torch_em_chunk(torch, x, nx[sel], y, ny[sel], 200, 1e-6)
            return pi, mu, it
        entry = {'what': what, 'npos': npos, 'computed': int(on.sum())}
        routes = [('new', new)]
        if not a.no_baselines:
            t_old, (opi, omu, oit) = event_time(torch, old)
            live = on[:tp] & ((out['status'][:tp] & (L.MIX_DEGENERATE | L.MIX_SKIPPED)) == 0)
            entry['torch_same_iters'] = float((oit[live] == out['iters'][:tp][live]).double().mean())
            same = live & (oit == out['iters'][:tp])
            entry['torch_max_pi_err'] = float((opi[same] - out['pi'][:tp][same]).abs().max()) if bool(same.any()) else 0.0
            entry['torch_max_mu_err'] = float((omu[same] - out['mu_mod'][:tp][same]).abs().max()) if bool(same.any()) else 0.0
            routes.append(('torch', old))
        times = {k: [] for k, _ in routes}
        for _ in range(a.reps):
            for k, fn in routes:
                times[k].append(event_time(torch, fn)[0])
        for k in times:
            entry[k + '_ms'] = float(np.median(times[k])); entry[k + '_min_ms'] = float(np.min(times[k]))
        work = float((ny[on].double() * out['iters'][on].double()).sum())
        entry['sample_iterations'] = work
        entry['positions_per_s'] = npos / (entry['new_ms'] * 1e-3)
        entry['computed_positions_per_s'] = entry['computed'] / (entry['new_ms'] * 1e-3)
        entry['exp_per_s'] = work / (entry['new_ms'] * 1e-3)
        entry['share_of_issue_bound'] = entry['exp_per_s'] / ISSUE_BOUND
        st = out['status']
        entry['not_converged'] = int(((st & L.MIX_NOT_CONVERGED) != 0).sum()); entry['mean_iters'] = float(out['iters'][on].double().mean())
        lines.append('%s: %s' % (name, what))
        lines.append('  computed %d of %d positions, mean %.1f iterations, %d at max_iter; %.3g sample-iterations'
                     % (entry['computed'], npos, entry['mean_iters'], entry['not_converged'], work))
        lines.append('  new    %10.3f ms (min %10.3f)  = %.3g positions/s (%.3g computed/s), %.3g exp/s = %.1f %% of the fp64-issue bound'
                     % (entry['new_ms'], entry['new_min_ms'], entry['positions_per_s'], entry['computed_positions_per_s'], entry['exp_per_s'],
                        100 * entry['share_of_issue_bound']))
        if not a.no_baselines:
            scale = npos / float(tp)
            entry['torch_positions'] = tp
            entry['torch_over_new'] = entry['torch_ms'] * scale / entry['new_ms']
            lines.append('  torch  %10.3f ms (min %10.3f) on %d positions%s = %.1f x the new entry; same iteration count at %.2f %% of the '
                         'positions, there |pi| differs by <= %.1e, |mu_mod| by <= %.1e'
                         % (entry['torch_ms'], entry['torch_min_ms'], tp, ' (scaled by %.1f)' % scale if tp != npos else '', entry['torch_over_new'],
                            100 * entry['torch_same_iters'], entry['torch_max_pi_err'], entry['torch_max_mu_err']))
        lines.append('')
        result['configs'][name] = entry

    n, reads = a.npos, a.reads
    sig0 = torch.empty(n * reads, dtype=torch.int16, device=dev); sig1 = torch.empty_like(sig0)
    det.synth_fill_events(sig0, a.seed, 0, n, 0, n_per_pos=reads, plant_period=100, plant_shift_milli=800, spread_milli=200)
    det.synth_fill_events(sig1, a.seed, 0, n, 1, n_per_pos=reads, plant_period=100, plant_shift_milli=800, spread_milli=200)
    measure('ungated', '%d x %d v %d event-like int16 rows, 3 %% planted at 4 sigma' % (n, reads, reads), n, sig0, sig1, None, None, reads, None)
    rid = torch.zeros(n, dtype=torch.int32, device=dev)
    res = det.run(sig0, sig1, rid, stride0=reads, stride1=reads, npos=n)
    (q,), _ = det.fdr(res, tracks=('comb_p',), method='bh', alpha=0.05)
    del res
    measure('gated', 'the same rows, gate = BH q of the combined track <= 0.05', n, sig0, sig1, None, None, reads, q)
    del sig0, sig1, q, rid
    torch.cuda.empty_cache()
    rn = a.ragged_npos
    g = torch.Generator(device=dev).manual_seed(a.seed)
    c0 = torch.randint(20, 401, (rn,), device=dev, generator=g); c1 = torch.randint(20, 401, (rn,), device=dev, generator=g)
    off0 = torch.zeros(rn + 1, dtype=torch.int64, device=dev); off1 = torch.zeros_like(off0)
    off0[1:] = torch.cumsum(c0, 0); off1[1:] = torch.cumsum(c1, 0)
    r0 = torch.empty(int(off0[-1]), dtype=torch.int16, device=dev); r1 = torch.empty(int(off1[-1]), dtype=torch.int16, device=dev)
    det.synth_fill_events(r0, a.seed, 0, rn, 0, off=off0, plant_period=100, plant_shift_milli=800, spread_milli=200)
    det.synth_fill_events(r1, a.seed, 0, rn, 1, off=off1, plant_period=100, plant_shift_milli=800, spread_milli=200)
    measure('ragged', '%d positions of 20 .. 400 reads per group (CSR), ungated' % rn, rn, r0, r1, off0, off1, 0, None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
