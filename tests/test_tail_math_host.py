"""CPU: the fp64 tail functions of special_math.hpp that K2 and K3 call per position, compiled for the host and held against
mpmath at tail_ref's precision.

A small stand-alone program is built with the host compiler: it includes nanomod_amd/csrc/special_math.hpp through a stub
<hip/hip_runtime.h> that defines the HIP qualifiers away, so glibc's exp / log / sqrt stand where the device has ocml's.  It is
the arithmetic of the functions that is checked here (series, powers, polynomials, guards), not the kernels: those are
tests/test_tails_gpu.py and tests/test_ks_tail_trim_gpu.py.

  * norm_isf (AS241 PPND16): 1e5 points, log-uniform from DBL_MIN to 0.5 and mirrored above 0.5, plus the end points;
    relative error in z <= 7e-13, the figure the Acklam + Newton form before it was documented with.
  * kolmogorov_sf (one exp per branch, the powers by multiplication): 1.2e4 points of 0.05 <= x <= 26 on both sides of the
    0.82 split; its worst error is no larger than that of the form with one exp per term (restated below) on the same points
    plus 1e-15.
  * the guards return exactly what they returned before."""
import math
import os
import shutil
import subprocess
import sys
from statistics import NormalDist

import numpy as np
import pytest

import tail_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nanomod_amd', 'csrc')
DBL_MIN = sys.float_info.min

STUB = r'''
#pragma once
#include <math.h>
#include <stdint.h>
#define __device__
#define __host__
#define __constant__
#define __forceinline__ inline
#define __ballot(x) ((unsigned long long)((x) ? 1 : 0))
#define __builtin_amdgcn_rcp(x) (1.0 / (x))
'''

MAIN = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "special_math.hpp"
// tailmath <function> <in> <out>: one double in, one double out, raw
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END); long n = ftell(f) / 8; fseek(f, 0, SEEK_SET);
  double* x = (double*)malloc(8 * (n > 0 ? n : 1));
  if (fread(x, 8, n, f) != (size_t)n) return 4;
  fclose(f);
  for (long i = 0; i < n; ++i) {
    if (!strcmp(argv[1], "norm_isf")) x[i] = nmod::norm_isf(x[i]);
    else if (!strcmp(argv[1], "kolmogorov_sf")) x[i] = nmod::kolmogorov_sf(x[i]);
    else return 5;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(x, 8, n, f) != (size_t)n) return 6;
  fclose(f);
  return 0;
}
'''


@pytest.fixture(scope='module')
def tailmath(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('tailmath')
    os.makedirs(d / 'stub' / 'hip')
    (d / 'stub' / 'hip' / 'hip_runtime.h').write_text(STUB)
    (d / 'main.cpp').write_text(MAIN)
    exe = str(d / 'tailmath')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-I', str(d / 'stub'), '-I', CSRC, str(d / 'main.cpp'), '-o', exe, '-lm'])

    def run(fn, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        x.tofile(str(d / 'in.bin'))
        subprocess.check_call([exe, fn, str(d / 'in.bin'), str(d / 'out.bin')])
        out = np.fromfile(str(d / 'out.bin'), dtype=np.float64)
        assert out.shape == x.shape
        return out
    return run


# ---------------------------------------------------------------------------------------------------------- norm_isf
N_LOW, N_MIRROR = 50000, 25000


def _isf_points():
    """q in (0, 0.5]: N_LOW log-uniform from DBL_MIN, N_MIRROR log-uniform from 2^-53 on the grid of 2^-53 (so that 1 - q is a
    double and the mirrored point is exactly p = 1 - q), and the end points"""
    rng = np.random.default_rng(241)
    low = np.exp(rng.uniform(math.log(DBL_MIN), math.log(0.5), N_LOW))
    low = np.clip(low, DBL_MIN, 0.5)
    low = np.concatenate([low, rng.uniform(0.075, 0.5, 4000)])   # (the central pair: where most p of a null-like track are)
    grid = np.exp(rng.uniform(math.log(2.0 ** -53), math.log(0.5), N_MIRROR))
    grid = np.clip(np.rint(grid * 2.0 ** 53), 1, 2.0 ** 52) * 2.0 ** -53
    ends = np.array([DBL_MIN, 0.075, np.nextafter(0.075, 0), math.exp(-25.0), np.nextafter(math.exp(-25.0), 1)])
    return np.concatenate([low, ends]), np.concatenate([grid, [2.0 ** -53, 0.25, 0.5]])


def _isf_reference(q):
    """z with Q(z) = q at tail_ref's precision: one Newton step on log Q(z) - log q (tail_ref.norm_isf_mp's iteration) from the
    standard library's inverse, which is itself good to a few 1e-16.  The step is quadratic: after a step of relative size s
    the error is of the order z^2 s^2, and s <= 1e-13 is asserted, so the reference is good to 1e-23 or better."""
    mp = T._mp()
    nd = NormalDist()
    s2pi = mp.sqrt(2 * mp.pi)
    ref = np.empty(len(q))
    for i, v in enumerate(q):
        v = float(v)
        if v == 0.5:
            ref[i] = 0.0
            continue
        z = mp.mpf(-nd.inv_cdf(v))
        Q = T.norm_sf_mp(z)
        step = (mp.log(Q) - mp.log(mp.mpf(v))) * Q * s2pi * mp.exp(z * z / 2)
        assert abs(step) <= mp.mpf(10) ** -13 * max(1, abs(z)), (v, step)
        ref[i] = float(z + step)
    return ref


def test_norm_isf_against_mpmath(tailmath):
    pytest.importorskip('mpmath')
    low, grid = _isf_points()
    q = np.concatenate([low, grid])
    ref = _isf_reference(q)
    # the one-step reference against tail_ref's converged iteration on a sample
    for i in range(0, len(q), 4999):
        assert abs(T.norm_isf_mp(float(q[i])) - ref[i]) <= 2.3e-16 * abs(ref[i]), q[i]
    z = tailmath('norm_isf', q)
    zm = tailmath('norm_isf', 1.0 - grid)                        # (exact: grid is on multiples of 2^-53)
    assert len(q) + len(grid) >= 100000
    assert (1.0 - (1.0 - grid) == grid).all()
    # p <= 0.5 never gives a negative z (the function has no clamp for it), p > 0.5 never a positive one; 0.5 gives +0
    assert (z >= 0.0).all() and (zm <= 0.0).all()
    assert z[q == 0.5].size and (z[q == 0.5] == 0.0).all() and not np.signbit(z[q == 0.5]).any()
    nz = ref != 0.0
    err = np.abs(z[nz] - ref[nz]) / ref[nz]
    refm = ref[len(low):]
    mz = refm != 0.0
    errm = np.abs(zm[mz] + refm[mz]) / refm[mz]
    for name, e, pts in (('p <= 0.5', err, q[nz]), ('p > 0.5', errm, grid[mz])):
        for lo, hi in ((0.075, 0.5), (math.exp(-25.0), 0.075), (0.0, math.exp(-25.0))):
            sel = (pts > lo) & (pts <= hi)
            if sel.any():
                print('  host norm_isf %-9s %.3g < q <= %.3g  n=%-6d worst rel %.2e' % (name, lo, hi, sel.sum(), e[sel].max()))
    # every branch of PPND16 is reached on both sides
    assert (q >= 0.075).sum() >= 100 and ((q < 0.075) & (q >= math.exp(-25.0))).sum() >= 1000 and (q < math.exp(-25.0)).sum() >= 1000
    assert (grid >= 0.075).sum() >= 100 and ((grid < 0.075) & (grid >= math.exp(-25.0))).sum() >= 1000 and (grid < math.exp(-25.0)).sum() >= 1000
    assert err.max() <= 7e-13, (err.max(), q[nz][err.argmax()])
    assert errm.max() <= 7e-13, (errm.max(), grid[mz][errm.argmax()])


# ------------------------------------------------------------------------------------------------------ kolmogorov_sf
def kolmogorov_sf_per_term(x):
    """the form that stood in special_math.hpp before: one exp per term of either series"""
    if not x > 0.0:
        return x if x != x else 1.0
    if x < 0.82:
        w = 1.2337005501361697 / (x * x)
        s = math.exp(-w) + math.exp(-9.0 * w) + math.exp(-25.0 * w) + math.exp(-49.0 * w)
        return 1.0 - 2.5066282746310002 / x * s
    q = -2.0 * x * x
    s, sign = 0.0, 1.0
    for k in range(1, 9):
        t = math.exp(q * float(k * k))
        s += sign * t
        sign = -sign
        if t < 1e-18 * s:
            break
    return 2.0 * s


def test_kolmogorov_sf_against_mpmath(tailmath):
    pytest.importorskip('mpmath')
    rng = np.random.default_rng(82)
    x = np.concatenate([rng.uniform(0.05, 0.82, 3000), rng.uniform(0.82, 2.0, 3000), rng.uniform(2.0, 26.0, 4000),
                        np.exp(rng.uniform(math.log(0.05), math.log(26.0), 2000)),
                        [0.05, np.nextafter(0.82, 0), 0.82, np.nextafter(0.82, 1), 18.0, 19.0, 26.0]])
    assert len(x) >= 10000 and (x < 0.82).sum() >= 3000 and (x >= 0.82).sum() >= 3000
    ref = np.array([float(T.kolmogorov_mp(float(v))) for v in x])
    new = tailmath('kolmogorov_sf', x)
    old = np.array([kolmogorov_sf_per_term(float(v)) for v in x])
    # as K2 hands them on: clamped at DBL_MIN (below it a double has no relative accuracy to speak of)
    clamp = lambda p: np.maximum(p, DBL_MIN)
    ref, new, old = clamp(ref), clamp(new), clamp(old)
    assert (ref == DBL_MIN).sum() >= 100 and np.array_equal(new == DBL_MIN, ref == DBL_MIN)
    e_new, e_old = np.abs(new - ref) / ref, np.abs(old - ref) / ref
    for name, sel in (('x < 0.82', x < 0.82), ('0.82 <= x < 2', (x >= 0.82) & (x < 2.0)), ('2 <= x', x >= 2.0)):
        print('  host kolmogorov_sf %-14s n=%-5d worst rel %.2e (one exp per term: %.2e)' % (name, sel.sum(), e_new[sel].max(), e_old[sel].max()))
        assert e_new[sel].max() <= e_old[sel].max() + 1e-15, (name, e_new[sel].max(), e_old[sel].max())


# ------------------------------------------------------------------------------------------------------------- guards
def test_guards_return_what_they_returned(tailmath):
    inf, nan = math.inf, math.nan
    k = tailmath('kolmogorov_sf', [0.0, -0.0, -1.0, -inf, nan, inf])
    assert list(k[:4]) == [1.0, 1.0, 1.0, 1.0] and np.isnan(k[4]) and k[5] == 0.0
    z = tailmath('norm_isf', [0.0, -0.0, -1.0, 1.0, 2.0, inf, nan, -inf])
    assert list(z[:3]) == [inf, inf, inf] and list(z[3:6]) == [-inf, -inf, -inf] and np.isnan(z[6]) and z[7] == inf
