"""CPU: the restatements of nmod_read_hmm (K19, tests/hmm_ref.py) against 60-digit mpmath within the derived gates, the limits the model
must reproduce (independence at a tiny correlation length, the closed form of two entries), the build rule, the bindings' layout, the
writers' formats and the derivation of the runs.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import hmm_ref as H
from nanomod_amd import _lib as L
from nanomod_amd import readllr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')


def _positions(rng, m, max_gap=40):
    return np.cumsum(rng.integers(1, max_gap + 1, m)).astype(np.float64)


def _scores(kind, rng, m):
    if kind == 'normal':
        return rng.normal(0.0, 3.0, m)
    if kind == 'blocks':
        return np.where((np.arange(m) // 7) % 2 == 0, -6.0, 6.0)
    return rng.choice(np.array([800.0, -800.0, 5.0, -5.0, 0.0, 40.0]), m)


CASES = [(1, 'normal', 0.3, 200.0), (1, 'extreme', 1e-6, 1e6), (2, 'normal', 0.5, 50.0), (130, 'normal', 0.2, 200.0), (130, 'extreme', 1e-6, 1e6),
         (257, 'blocks', 0.1, 100.0), (300, 'extreme', 0.4, 30.0), (400, 'blocks', 1e-6, 1e6), (400, 'normal', 0.7, 1e6),
         (H.WAVE_MAX + 1, 'blocks', 0.3, 150.0), (5000, 'normal', 0.05, 400.0), (5000, 'extreme', 1e-6, 1e6)]


def check_against_mp(res, exact, m):
    """post within G ref + 1e-290, ll and ll_indep within G (D + 1); returns the largest relative errors seen (post, ll)"""
    import mpmath as mp
    g = H.gate(m)
    worst = 0.0
    with mp.workdps(60):
        for j in range(m):
            err = abs(mp.mpf(float(res['post'][j])) - exact['post'][j])
            assert err <= g * exact['post'][j] + mp.mpf(H.FLOOR), (j, float(res['post'][j]), float(exact['post'][j]))
            if exact['post'][j] > 1e-280:
                worst = max(worst, float(err / exact['post'][j]))
        d = exact['denom']
        errs = [abs(mp.mpf(res[f]) - exact[f]) for f in ('ll', 'll_indep')]
        assert all(e <= g * (d + 1) for e in errs), [float(e / (d + 1)) for e in errs]
    return worst, float(max(errs) / (d + 1))


@pytest.mark.parametrize('m,kind,pi,length', CASES)
def test_both_restatements_against_mpmath(m, kind, pi, length):
    rng = np.random.default_rng(1900 + m)
    x, s = _positions(rng, m), _scores(kind, rng, m)
    exact = H.hmm_mp(x, s, pi, length)
    for chain in (H.hmm_seq, H.hmm_device_order):
        worst, worst_ll = check_against_mp(chain(x, s, pi, length), exact, m)
        assert worst < 1e-13 and worst_ll < 1e-13                 # (far inside the cap: the chain forgets)


def test_the_gate_is_capped_and_grows_from_the_roundings():
    assert H.STEP_U == 29 and H.path_u(1) == 28 and H.path_u(4) == 88
    assert H.gate(1) == H.U * (2 * (29 * 2 + 2 * 28) + 4) < 3e-14
    assert H.gate(50) < H.gate(100) < H.CAP == H.gate(200) == H.gate(5000) == 1e-12
    assert H.threads(H.WAVE_MAX) == 64 and H.threads(H.WAVE_MAX + 1) == 256


def test_a_tiny_length_is_independence():
    rng = np.random.default_rng(1901)
    m, pi = 90, 0.23
    x, s = _positions(rng, m), rng.normal(0.0, 3.0, m)
    g = H.gate(m)
    for chain in (H.hmm_seq, H.hmm_device_order):
        res = chain(x, s, pi, 1e-3)                               # rho = exp(-1000 d) = 0: every row of T is (q, pi)
        want = np.array([pi * math.exp(min(v, 0.0)) / ((1.0 - pi) * math.exp(-max(v, 0.0)) + pi * math.exp(min(v, 0.0))) for v in s])
        assert np.all(H.post_within(res['post'], want, g))
        denom = H.hmm_seq(x, s, pi, 1e-3)['denom']
        assert abs(res['ll'] - res['ll_indep']) <= 2 * g * (denom + 1)      # (each within its gate of the common value)


def test_two_entries_against_the_closed_form():
    import mpmath as mp
    pi, length, d = 0.3, 25.0, 10.0
    for s0, s1 in ((2.0, -1.0), (-4.0, 6.0), (0.0, 0.0), (800.0, -800.0)):
        with mp.workdps(60):
            q = mp.mpf(1.0 - pi)
            p = [q, mp.mpf(pi)]
            r = mp.mpf(d) / mp.mpf(length)
            rho, eps = mp.exp(-r), -mp.expm1(-r)
            T = [[q + p[1] * rho, p[1] * eps], [q * eps, p[1] + q * rho]]
            e = [[mp.exp(-max(mp.mpf(v), 0)), mp.exp(min(mp.mpf(v), 0))] for v in (s0, s1)]
            joint = [[p[a] * e[0][a] * T[a][b] * e[1][b] for b in (0, 1)] for a in (0, 1)]
            tot = sum(sum(row) for row in joint)
            want = [float((joint[1][0] + joint[1][1]) / tot), float((joint[0][1] + joint[1][1]) / tot)]
            want_ll = float(mp.log(tot) + max(s0, 0.0) + max(s1, 0.0))
        for chain in (H.hmm_seq, H.hmm_device_order):
            res = chain(np.array([100.0, 100.0 + d]), np.array([s0, s1]), pi, length)
            assert np.all(H.post_within(res['post'], want, H.gate(2))), (s0, s1, res['post'], want)
            assert H.ll_within(res['ll'], want_ll, H.gate(2), H.hmm_seq(np.array([100.0, 100.0 + d]), np.array([s0, s1]), pi, length)['denom'])


def test_an_invalid_score_is_skipped_with_the_larger_gap():
    key = np.array([(0 << 40) | p for p in (10, 20, 30)], np.int64)
    cs, start, roff = np.array([0], np.int32), np.array([5], np.int64), np.array([0, 40], np.int64)
    score = np.zeros(40)
    score[[5, 15, 25]] = 3.0, np.nan, -2.0
    hoff, site, x, s = H.entries_ref(cs, start, roff, score, key)
    assert hoff.tolist() == [0, 2] and site.tolist() == [0, 2] and x.tolist() == [10.0, 30.0] and s.tolist() == [3.0, -2.0]
    score[:] = 0.0
    score[5 + 40 - 1 - 30] = 7.0                                  # '-': event i lies at start + n - 1 - i, so position 30 is event 14
    hoff, site, x, s = H.entries_ref(np.array([1], np.int32), start, roff, score, key + (1 << 40))
    assert site.tolist() == [0, 1, 2] and s.tolist() == [0.0, 0.0, 7.0]


def test_header_constants_bindings_and_build_rule():
    text = open(HEADER).read()
    assert int(re.search(r'#define NMOD_HMM_CHUNK (\d+)', text).group(1)) == H.CHUNK == L.HMM_CHUNK
    assert int(re.search(r'#define NMOD_HMM_WAVE_MAX (\d+)', text).group(1)) == H.WAVE_MAX == L.HMM_WAVE_MAX
    assert 'enum { NMOD_HMM_NO_SITE = 1 };' in text and L.HMM_NO_SITE == H.NO_SITE == 1
    assert '#define NMOD_ABI_VERSION 4' in text
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu", sizeof(nmod_hmm_opts), ' \
          'offsetof(nmod_hmm_opts, call_post), sizeof(nmod_hmm_out), offsetof(nmod_hmm_out, post), offsetof(nmod_hmm_out, n_sites), ' \
          'offsetof(nmod_hmm_out, status), offsetof(nmod_hmm_out, site_can));return 0;}' % HEADER
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == [C.sizeof(L.NmodHmmOpts), L.NmodHmmOpts.call_post.offset, C.sizeof(L.NmodHmmOut), L.NmodHmmOut.post.offset, L.NmodHmmOut.n_sites.offset,
                   L.NmodHmmOut.status.offset, L.NmodHmmOut.site_can.offset] == [32, 24, 112, 8, 32, 80, 104]
    lib = L.load()
    for name in ('nmod_read_sites_count', 'nmod_read_hmm'):
        assert name in L._SIGNATURES and getattr(lib, name).argtypes is not None
    csrc = os.path.join(ROOT, 'nanomod_amd', 'csrc')
    src = open(os.path.join(csrc, 'read_hmm.hip')).read()
    assert '#include "read_walk.hpp"' in src and '#include "site_search.hpp"' in src and 'draw_read<WAVES>' in src and 'sp_bound<' in src
    pairs = open(os.path.join(csrc, 'site_pairs.hip')).read()
    assert '#include "site_search.hpp"' in pairs and 'int64_t sp_bound(' not in pairs + src       # one copy of the search, in the header
    code = re.sub(r'//.*', '', src)
    assert not re.search(r'atomicAdd\(\s*\(?\s*(double|float)', code) and 'atomicAdd(&o.site_' in code    # integer atomics on the site counts only
    mk = open(os.path.join(csrc, 'Makefile')).read()              # contraction off for the unit: its target-specific flag, used by the one .hip rule
    assert re.search(r'^\$\(OBJDIR\)/read_hmm\.o: CXXFLAGS \+= -ffp-contract=off$', mk, re.M)
    assert re.search(r'^\$\(OBJDIR\)/%\.o: %\.hip .*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -c', mk, re.M) and 'read_hmm.o' in re.search(r'^OBJS\s*=((?:.*\\\n)*.*)$', mk, re.M).group(1)


def test_runs_of_a_constructed_state_track():
    #        read 0: 5 entries        read 1: none   read 2: 4 entries     read 3: 1
    state = np.array([1, 1, 2, 1, 0,                  1, 1, 1, 1,           1], np.uint8)
    hoff = np.array([0, 5, 5, 9, 10], np.int64)
    post = np.array([0.95, 0.99, 0.5, 0.91, 0.01, 1.0, 0.92, 0.93, 0.94, 0.9])
    site = np.array([0, 1, 2, 3, 4, 1, 2, 3, 4, 0], np.int32)
    site_pos = np.array([100, 110, 125, 130, 170], np.int64)
    first, last = H.runs(state[0:5])
    assert first.tolist() == [0, 3] and last.tolist() == [1, 3]
    assert H.per_read(hoff, state)['n_runs'].tolist() == [2, 0, 1, 1] and H.per_read(hoff, state)['n_mod'].tolist() == [3, 0, 4, 1]
    d = readllr.read_domains(hoff, site, state, post, site_pos)
    assert d['read'].tolist() == [0, 0, 2, 3]                     # runs do not join across the boundary of reads 0 | 2 | 3
    assert d['first'].tolist() == [100, 130, 110, 100] and d['last'].tolist() == [110, 130, 170, 100] and d['n_sites'].tolist() == [2, 1, 4, 1]
    assert np.allclose(d['mean_post'], [0.97, 0.91, (1.0 + 0.92 + 0.93 + 0.94) / 4, 0.9], rtol=1e-15)
    empty = readllr.read_domains(np.array([0, 2]), site[:2], np.array([0, 2], np.uint8), post[:2], site_pos)
    assert all(len(v) == 0 for v in empty.values())
    sites = H.per_site(site, state, 5)
    assert sites['site_n'].tolist() == [2, 2, 2, 2, 2] and sites['site_mod'].tolist() == [2, 2, 1, 2, 1] and sites['site_can'].tolist() == [0, 0, 0, 0, 1]
    assert H.states([0.9, 0.09999999999999998, 0.1, 0.5, float('nan'), 0.0, 1.0], 0.9).tolist() == [1, 0, 2, 2, 2, 0, 1]   # 1 - 0.9 is 0.09999999999999998


def test_writer_formats():
    res = dict(reads=dict(index=np.array([0, 1]), chrom=np.array(['chrA', 'chrB']), strand=np.array(['+', '-']), n_sites=np.array([3, 0], np.int32),
                          n_mod=np.array([2, 0], np.int32), n_can=np.array([1, 0], np.int32), n_runs=np.array([1, 0], np.int32),
                          ll=np.array([-1.25, 0.0]), ll_indep=np.array([-2.5, 0.0]), status=np.array([0, 1], np.uint8)),
               domains=dict(read=np.array([0]), first=np.array([99]), last=np.array([149]), n_sites=np.array([2]), mean_post=np.array([0.9876543])),
               sites=dict(chrom=np.array(['chrA', 'chrA']), strand=np.array(['+', '+']), pos=np.array([99, 149]), n=np.array([1, 1], np.int32),
                          n_mod=np.array([1, 0], np.int32), n_can=np.array([0, 0], np.int32), share=np.array([1.0, np.nan])))
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, n) for n in ('a', 'b', 'c')]
        readllr.write_read_hmm(paths[0], res); readllr.write_read_domains(paths[1], res); readllr.write_site_hmm(paths[2], res)
        assert open(paths[0]).read() == '0 chrA + 3 2 1 1 -1.250000 -2.500000 2.500000\n1 chrB - 0 0 0 0 0.000000 0.000000 0.000000\n'
        assert open(paths[1]).read() == '0 chrA + 100 150 2 0.987654\n'
        assert open(paths[2]).read() == 'chrA + 100 1 1 0 1.000000\nchrA + 150 1 0 0 nan\n'


def test_the_python_layer_refuses_what_the_entry_refuses():
    from nanomod_amd import cli, engine
    for kw in (dict(pi=0.0), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=2e9), dict(length=float('inf')),
               dict(call_post=0.5), dict(call_post=1.0), dict(call_post=float('nan')), dict(want=('post', 'nope'))):
        with pytest.raises(ValueError):
            engine._hmm_opts(*[dict(dict(pi=0.3, length=200.0, call_post=0.9, want=()), **kw)[k] for k in ('pi', 'length', 'call_post', 'want')])
    a = cli.build_parser().parse_args(['readhmm', '--wrkBase1', HEADER, '--model', HEADER, '--altModel', HEADER, '--hmmPi', '2', '--hmmLength', '0',
                                       '--fitLength', '50,x', '--callPost', '0.4'])
    errs = cli.validate_readhmm(a)
    assert len(errs) == 4 and all(('--' + o) in e for o, e in zip(('hmmPi', 'hmmLength', 'fitLength', 'callPost'), errs))
    assert cli.parse_fit_length('50,100,200') == [50.0, 100.0, 200.0] and cli.parse_fit_length('') is None
