"""CPU: the restatements of nmod_read_viterbi (K20, tests/viterbi_ref.py): the sequential recursion against a brute force over all paths,
both float64 restatements against 60-digit mpmath within the derived gates, vit <= ll against hmm_ref, the share of entries path equality
leaves out on the constructed fixtures, the header's constants and layouts, the build rule, the argument layer's refusals, the command
line's option and the writers.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import hmm_ref as H
import viterbi_ref as V
from nanomod_amd import _lib as L
from nanomod_amd import readllr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
GRID_SCORES = np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, 0.0, 40.0, -7.5])     # K19's score grid, its valid values


def _positions(rng, m, max_gap=40):
    return np.cumsum(rng.integers(1, max_gap + 1, m)).astype(np.float64)


def test_sequential_equals_brute_force_for_every_small_read():
    """every m <= 12: the recursion's path reaches the largest score of all 2^m paths (to the roundings of m sums), and is the one path
    that does where there is one; pi = 0.5 with every score 0 ties state 0 and state 1 throughout: the recursion gives all 0"""
    rng = np.random.default_rng(2001)
    for m in range(1, 13):
        for pi, length, ties in ((0.3, 30.0, False), (0.7, 5.0, False), (0.5, 30.0, True)):
            x = _positions(rng, m, 20)
            s = np.zeros(m) if ties else rng.choice(GRID_SCORES, m)
            res = V.viterbi_seq(x, s, pi, length)
            best, paths = V.brute_force(x, s, pi, length)
            slack = 4 * (m + 2) * V.U * (V.scale(x, s, pi, length) + 1.0)     # the recursion's m + 1 sums against an exactly rounded sum
            assert abs(res['vit'] - best) <= slack and abs(V.path_score(res['path'], x, s, pi, length) - best) <= slack, (m, pi)
            if len(paths) == 1:
                assert res['path'].tolist() == paths[0], (m, pi)
            if ties:
                assert res['path'].tolist() == [0] * m and [0] * m in paths and [1] * m in paths
            assert np.all((res['delta'] >= -slack) | (res['path'] == 0)) and np.all((res['delta'] <= slack) | (res['path'] == 1))


CASES = [(1, 0.3, 200.0), (2, 0.5, 50.0), (5, 1e-9, 1e6), (130, 0.2, 200.0), (257, 0.1, 100.0), (300, 1.0 - 1e-9, 200.0), (400, 0.3, 1e-3),
         (H.WAVE_MAX + 1, 0.3, 150.0), (2 * 1024 * 2 + 3, 0.3, 1e6)]


@pytest.mark.parametrize('m,pi,length', CASES)
def test_both_restatements_against_mpmath(m, pi, length):
    """the path of either restatement, scored exactly, is within the gate of the optimum, vit and delta within the gate of the exact ones,
    the path the exact one wherever the exact |delta| exceeds the gate, and no entry of these fixtures is left out by that"""
    rng = np.random.default_rng(2000 + m)
    x = _positions(rng, m)
    s = rng.choice(GRID_SCORES, m) if m % 2 else np.round(rng.normal(0.0, 3.0, m), 3)
    c = V.MpChain(x, s, pi, length)
    g = V.gate(m) * (c.scale + 1.0)
    near, loss = c.near(g)
    assert (near, loss) == (0, 0.0) and np.all(np.abs(c.delta) > g)
    assert np.min(np.abs(c.delta)) > 1e3 * g                                  # (the smallest gap is orders above the gate)
    for chain in (V.viterbi_seq, V.viterbi_device_order):
        res = chain(x, s, pi, length)
        assert float(c.opt - c.path_score_mp(res['path'])) <= g
        assert abs(res['vit'] - float(c.opt)) <= g and np.all(np.abs(res['delta'] - c.delta) <= g)
        assert res['path'].tolist() == c.path.tolist() and np.all(res['path'] == (res['delta'] > 0))
    assert V.viterbi_device_order(x, s, pi, length)['vit'] <= H.hmm_device_order(x, s, pi, length)['ll'] + g


def test_the_gate_counts_roundings():
    assert V.path_v(1) == 14 and V.path_v(4) == 44 and V.STEP_U == 38
    assert V.gate(1) == V.gate(256) == V.U * (2 * (38 + 4 + 14) + (4 + 8 + 1) + 6) < 2e-14
    assert V.gate(257) == V.U * (2 * (42 + 2 * 14) + (8 + 8 + 1) + 6) and V.gate(H.WAVE_MAX) < V.gate(H.WAVE_MAX + 1) < V.gate(4099) < 1e-13 < V.CAP
    assert V.gate(10 ** 6) == V.CAP == H.CAP
    x, s = np.array([5.0, 6.0, 9.0]), np.array([2.0, -3.0, 0.0])
    assert V.scale(x, s, 0.3, 10.0) >= 3 * V.LN2 and abs(V.scale(x, s, 0.3, 10.0) - V.MpChain(x, s, 0.3, 10.0).scale) < 1e-12


def test_vit_is_at_most_ll_and_the_half_score_ties_follow_the_strict_rule():
    rng = np.random.default_rng(2002)
    for m, pi, length in ((1, 0.5, 10.0), (7, 0.3, 30.0), (200, 0.1, 100.0), (300, 0.8, 1e6)):
        x, s = _positions(rng, m), rng.normal(0.0, 3.0, m)
        ll = H.hmm_seq(x, s, pi, length)
        for chain in (V.viterbi_seq, V.viterbi_device_order):
            assert chain(x, s, pi, length)['vit'] <= ll['ll'] + H.gate(m) * (ll['denom'] + 1.0)
    # +s then -s at pi = 0.5, equal gaps: the mirror image has the mirrored scores of every path, so state 0 and state 1 tie at the last entry
    for m in (2, 8, 300):
        x = np.arange(m, dtype=np.float64) * 7.0
        a, b = (V.viterbi_seq(x, V.half_scores(m, 4.0, first), 0.5, 30.0) for first in (True, False))
        assert a['path'].tolist() == [1] * (m // 2) + [0] * (m - m // 2) and b['path'].tolist() == [0] * (m // 2) + [1] * (m - m // 2)
        assert a['vit'] == b['vit']
    zero = V.viterbi_seq(np.arange(9.0), np.zeros(9), 0.5, 30.0)
    assert zero['path'].tolist() == [0] * 9 and np.all(zero['delta'] == 0.0)


def test_header_constants_bindings_and_build_rule():
    text = open(HEADER).read()
    assert '#define NMOD_ABI_VERSION 4' in text and 'no Viterbi' not in text and 'nmod_read_viterbi' in text
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu", sizeof(nmod_vit_opts), ' \
          'offsetof(nmod_vit_opts, length), sizeof(nmod_vit_out), offsetof(nmod_vit_out, path), offsetof(nmod_vit_out, delta), ' \
          'offsetof(nmod_vit_out, n_sites), offsetof(nmod_vit_out, status), offsetof(nmod_vit_out, site_mod));return 0;}' % HEADER
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, 't')]).split()]
    O = L.NmodVitOut
    assert got == [C.sizeof(L.NmodVitOpts), L.NmodVitOpts.length.offset, C.sizeof(O), O.path.offset, O.delta.offset, O.n_sites.offset, O.status.offset,
                   O.site_mod.offset] == [24, 16, 88, 8, 24, 32, 64, 80]
    assert L.VIT_ENTRY_FIELDS == ('path', 'site', 'delta') and L.VIT_READ_FIELDS == ('n_sites', 'n_mod', 'n_runs', 'vit', 'status')
    assert L.VIT_SITE_FIELDS == ('site_n', 'site_mod') and V.CHUNK == L.HMM_CHUNK and V.WAVE_MAX == L.HMM_WAVE_MAX
    lib = L.load()
    assert 'nmod_read_viterbi' in L._SIGNATURES and lib.nmod_read_viterbi.argtypes is not None and lib.nmod_abi_version() == 4
    csrc = os.path.join(ROOT, 'nanomod_amd', 'csrc')
    code = re.sub(r'//.*', '', open(os.path.join(csrc, 'read_viterbi.hip')).read())
    # the fill of the entries is enqueued by read_entries.hpp's ChainCall, for every chain entry: one copy of that call
    shared = re.sub(r'//.*', '', open(os.path.join(csrc, 'read_entries.hpp')).read())
    assert '#include "read_entries.hpp"' in code and 'draw_read<WAVES>' in code and 'ChainCall c(' in code
    assert shared.count('rh_fill_entries(e, num_cus, stream)') == 1 and 'rh_fill_entries(' not in code
    assert 'rh_fill_entries(' not in re.sub(r'//.*', '', open(os.path.join(csrc, 'read_classes.hip')).read())
    assert 'rh_entries_kernel' not in code and 'frexp' not in code and 'ldexp' not in code      # one copy of the entries' kernel; nothing is rescaled
    assert not re.search(r'atomicAdd\(\s*\(?\s*(double|float)', code) and 'atomicAdd(&o.site_' in code
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert re.search(r'^\$\(OBJDIR\)/read_viterbi\.o: CXXFLAGS \+= -ffp-contract=off$', mk, re.M)
    assert 'read_viterbi.o' in re.search(r'^OBJS\s*=((?:.*\\\n)*.*)$', mk, re.M).group(1)


def test_the_python_layer_refuses_what_the_entry_refuses():
    from nanomod_amd import cli, engine
    for kw in (dict(pi=0.0), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=2e9), dict(length=float('inf')),
               dict(want=('path', 'post'))):
        with pytest.raises(ValueError):
            engine._vit_opts(*[dict(dict(pi=0.3, length=200.0, want=()), **kw)[k] for k in ('pi', 'length', 'want')])
    opts, want = engine._vit_opts(0.25, 50.0, ('vit', 'path'))
    assert (opts.struct_size, opts.pi, opts.length, want) == (24, 0.25, 50.0, ('vit', 'path'))
    assert engine._vit_shapes(('vit', 'path', 'site_n'), 7, 3, 5) == dict(path=('uint8', 7), vit=('float64', 3), site_n=('int32', 5))
    cs, start, roff, key = np.zeros(1, np.int32), np.zeros(1, np.int64), np.array([0, 3], np.int64), np.array([1], np.int64)
    for bad in (dict(hoff=np.array([1, 1], np.int64)), dict(hoff=np.array([0, 1, 2], np.int64)), dict(pi=2.0), dict(want=('nope',))):
        with pytest.raises(ValueError):                                       # (refused before the library is asked for a device)
            engine.read_viterbi_host(cs, start, roff, np.zeros(3), key, **dict(dict(hoff=np.array([0, 1], np.int64)), **bad))
    with pytest.raises(ValueError):
        readllr.smooth_reads_llr(None, None, None, decode='map')


def test_the_command_line_option_and_the_default(monkeypatch):
    from nanomod_amd import cli, container, kmermodel
    base = ['readhmm', '--wrkBase1', HEADER, '--model', HEADER, '--altModel', HEADER, '--sites', HEADER]
    p = cli.build_parser()
    assert p.parse_args(base).decode == 'posterior'
    assert [p.parse_args(base + ['--decode', v]).decode for v in ('posterior', 'viterbi', 'both')] == ['posterior', 'viterbi', 'both']
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--decode', 'map'])
    assert inspect.signature(readllr.smooth_reads_llr).parameters['decode'].default == 'posterior'

    # with the default the call the command line makes is the one it has always made: no new argument reaches smooth_reads_llr
    class Stop(Exception):
        pass
    seen = {}

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop
    monkeypatch.setattr(container, 'load_reads', lambda path: None)
    monkeypatch.setattr(kmermodel, 'load_kmer_model', lambda path: None)
    monkeypatch.setattr(readllr, 'read_sites_file', lambda path: None)
    monkeypatch.setattr(readllr, 'smooth_reads_llr', fake)
    for argv, want in ((base, None), (base + ['--decode', 'posterior'], None), (base + ['--decode', 'both'], 'both'), (base + ['--decode', 'viterbi'], 'viterbi')):
        seen.clear()
        with pytest.raises(Stop):
            cli.run_readhmm(p.parse_args(argv))
        assert seen.get('decode') == want and ('decode' in seen) == (want is not None) and seen['call_post'] == 0.9


def test_domains_of_a_path_and_the_writers():
    #       read 0: 5 entries   read 1: none   read 2: 3 entries
    path = np.array([1, 1, 0, 1, 0,                1, 1, 1], np.uint8)
    delta = np.array([2.5, 0.25, -3.0, 1.0, -0.5, 4.0, 0.125, 9.0])
    hoff = np.array([0, 5, 5, 8], np.int64)
    site = np.array([0, 1, 2, 3, 4, 1, 2, 3], np.int32)
    pos = np.array([100, 110, 125, 130, 170], np.int64)
    d = readllr.read_domains(hoff, site, path, None, pos, delta=delta)
    assert d['read'].tolist() == [0, 0, 2] and d['first'].tolist() == [100, 130, 110] and d['last'].tolist() == [110, 130, 130]
    assert d['min_delta'].tolist() == [0.25, 1.0, 0.125] and np.all(np.isnan(d['mean_post'])) and d['n_sites'].tolist() == [2, 1, 3]
    post = np.linspace(0.1, 0.8, 8)
    both = readllr.read_domains(hoff, site, path, post, pos, delta=delta)
    assert np.allclose(both['mean_post'], [0.15, 0.4, 0.7], rtol=1e-15) and both['min_delta'].tolist() == d['min_delta'].tolist()
    assert set(readllr.read_domains(hoff, site, path, post, pos)) == {'read', 'first', 'last', 'n_sites', 'mean_post'}      # K19's keys as they are
    empty = readllr.read_domains(np.array([0, 2]), site[:2], np.zeros(2, np.uint8), None, pos, delta=delta[:2])
    assert all(len(v) == 0 for v in empty.values()) and 'min_delta' in empty
    assert V.per_read(hoff, path)['n_runs'].tolist() == [2, 0, 1] and V.per_site(site, path, 5)['site_mod'].tolist() == [1, 2, 1, 2, 0]
    res = dict(reads=dict(index=np.arange(3), chrom=np.array(['chrA', 'chrA', 'chrB']), strand=np.array(['+', '+', '-'])),
               entries=dict(hoff=hoff, site=site, path=path, delta=delta), domains=both,
               sites=dict(chrom=np.array(['chrA'] * 5), strand=np.array(['+'] * 5), pos=pos, n=np.array([1, 2, 2, 2, 1], np.int32),
                          n_mod=np.array([1, 2, 1, 2, 0], np.int32), share=np.array([1.0, 1.0, 0.5, 1.0, 0.0])))
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, n) for n in ('a', 'b', 'c')]
        readllr.write_read_viterbi(paths[0], res); readllr.write_read_domains(paths[1], res); readllr.write_site_viterbi(paths[2], res)
        rows = open(paths[0]).read().splitlines()
        assert rows[0] == '0 0 chrA + 101 1 2.500000' and rows[2] == '0 2 chrA + 126 0 -3.000000' and rows[5] == '2 1 chrA + 111 1 4.000000' and len(rows) == 8
        assert open(paths[1]).read() == '0 chrA + 101 111 2 0.150000 0.250000\n0 chrA + 131 131 1 0.400000 1.000000\n2 chrB - 111 131 3 0.700000 0.125000\n'
        assert open(paths[2]).read().splitlines()[2] == 'chrA + 126 2 1 0.500000'
