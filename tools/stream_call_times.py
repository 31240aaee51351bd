"""Host-side wall time of one call of every builder of tests/stream_cases.py (the twelve secondary NMOD_MEM_DEVICE entries and
nmod_detect_batch outside its exceptions), warm, on the shapes the stream-contract tests use: median, minimum and maximum of
--repeats calls, the stream synchronised between them.  The stall of tests/test_stream_contract_gpu.py (stream_cases.T_MS) is at least
50 times the slowest median, rounded up; profiles/stream_contract.txt keeps the table this prints.

    python tools/stream_call_times.py [--repeats 20] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import stream_cases as S
    from nanomod_amd import engine
    det = engine.DeviceDetector(0)
    lines = ['# host wall time of one call, ms: median / min / max of %d warm calls; %s' % (a.repeats, torch.cuda.get_device_name(0)),
             '%-16s %9s %9s %9s' % ('entry', 'median', 'min', 'max')]
    slowest = 0.0
    for b in S.BUILDERS:
        d = b.make_inputs(1)
        sw = S.Swapped(d['real'], d['decoy'])
        sw.load_real()
        out = b.call(det, sw.t)
        for _ in range(3):
            b.call(det, sw.t, out)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            b.call(det, sw.t, out)
            ms.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
        med = statistics.median(ms)
        slowest = max(slowest, med)
        lines.append('%-16s %9.3f %9.3f %9.3f' % (b.name, med, min(ms), max(ms)))
    kind, per, _ = S._calibrate(torch, torch.device('cuda:0'))
    lines.append('# slowest median %.3f ms; 50 x = %.1f ms; T_MS >= %d' % (slowest, 50 * slowest, int(math.ceil(50 * slowest / 10.0) * 10)))
    lines.append('# stall calibration: %s, %.3e ms per unit; stream_cases.T_MS = %g, cap %g ms' % (kind, per, S.T_MS, S.STALL_CAP_MS))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
