"""nmod_pair_index / nmod_site_pairs (K16) without a GPU: the restatement of the header's definition (tests/pairs_ref.py) — the double
recurrence of p_fisher in both orders against exact rational arithmetic within the gate it derives, and against scipy —, the pair index
and the counts on constructed cases, the declarations and struct layouts, and the refusals of every layer before any device work."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import pairs_ref as P
import readllr_ref as RF
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL
from nanomod_amd.engine import pair_index_host, site_pairs_host             # K16's entries: without them nothing here can pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
NO_DEVICE = 10 ** 6                                                           # a device that does not exist: a call that reaches it fails

# the large tables of the GPU tests as well: a support at and just past the thread form's limit, margins about 2 000 with p about
# 1e-111, and one whose p underflows
LARGE_TABLES = [(32, 31, 31, 32), (32, 32, 32, 32), (1351, 649, 649, 1351), (3000, 0, 0, 3000)]


def _support(t):
    _, _, _, lo, hi, _ = P.margins(*t)
    return hi - lo + 1


def _check_against_exact(t, worst):
    assert not P.near_tie(*t), t
    exact = P.fisher_exact(*t)
    for order, f in (('thread', P.fisher_thread), ('wave', P.fisher_wave)):
        p = f(*t)
        if exact < Fraction(1e-290):
            assert P.DBL_MIN <= p <= 1e-289, (order, t, p)
            continue
        dev = abs(Fraction(p) / exact - 1)
        L_ = _support(t)
        # (either order within the gate of its own class: the wave's further term applies to the wave's order at any L)
        assert dev <= Fraction(P.gate(L_, thread_max=0 if order == 'wave' else 10 ** 9)), (order, t, p, float(exact))
        worst[order] = max(worst.get(order, 0.0), float(dev / Fraction(P.U)) / L_)


def test_exhaustive_small_tables_against_exact_arithmetic():
    """every table with N <= 12, both orders of the recurrence; none of them is a near tie of the slack rule"""
    worst, n = {}, 0
    for N in range(0, 13):
        for n11 in range(N + 1):
            for n10 in range(N + 1 - n11):
                for n01 in range(N + 1 - n11 - n10):
                    _check_against_exact((n11, n10, n01, N - n11 - n10 - n01), worst)
                    n += 1
    print('%d tables; worst deviation in units of L u: %s' % (n, worst))


def test_large_tables_against_exact_arithmetic():
    worst = {}
    for t in LARGE_TABLES:
        _check_against_exact(t, worst)
    assert (_support(LARGE_TABLES[0]), _support(LARGE_TABLES[1])) == (L.PAIRS_THREAD_MAX, L.PAIRS_THREAD_MAX + 1)
    assert 1e-112 < float(P.fisher_exact(*LARGE_TABLES[2])) < 1e-110
    assert P.fisher_exact(*LARGE_TABLES[3]) < Fraction(1e-320) and P.fisher_recurrence(*LARGE_TABLES[3]) == P.DBL_MIN
    print('worst deviation in units of L u: %s' % worst)


def test_random_tables_against_scipy():
    """300 random tables with cells up to 5, 40 and 400: within 1e-12 relative of scipy.stats.fisher_exact wherever neither the
    definition's slack (1 + 1e-7) nor a tie slack anywhere between it and exact equality decides a table (scipy's own lies there)"""
    scipy_stats = pytest.importorskip('scipy.stats')
    rng = random.Random(1601)
    used = 0
    for i in range(300):
        m = (5, 40, 400)[i % 3]
        t = tuple(rng.randint(0, m) for _ in range(4))
        w, lo = P.exact_weights(*t)
        wo = w[t[0] - lo]
        if any(wo < v <= wo * (Fraction(P.SLACK) + Fraction(1e-9)) for v in w):            # a weight just above w(n11): whose slack decides
            continue
        used += 1
        want = scipy_stats.fisher_exact([[t[0], t[1]], [t[2], t[3]]])[1]
        got = P.fisher_recurrence(*t)
        assert abs(got - want) <= 1e-12 * want, (t, got, want)
    assert used >= 250, used


def test_pair_statistics_known_answers():
    r = P.pair_stats_ref(np.array([3, 1, 1, 3, 0, 0, 4, 4, 1, 1, 0, 0], np.int32), min_reads=3, poff=np.array([0, 2, 3, 3]))
    assert abs(r['log_or'][0] - np.log(3.5 * 3.5 / (1.5 * 1.5))) < 1e-15 and abs(r['phi'][0] - 0.5) < 1e-15
    assert abs(r['p_fisher'][0] - float(Fraction(2 * (1 + 16), 70))) < 1e-15                 # 2 (C(4,4) C(4,0) + C(4,3) C(4,1)) / C(8,4)
    assert r['status'].tolist() == [0, P.DEGENERATE, P.TOO_FEW | P.DEGENERATE]
    assert np.isnan(r['phi'][1]) and r['p_fisher'][1] == 1.0 and np.isfinite(r['log_or'][1]) and np.isfinite(r['se'][1])
    assert all(np.isnan(r[f][2]) for f in ('log_or', 'se', 'phi', 'p_fisher'))
    assert r['first'].tolist() == [0, 0, 1] and r['second'].tolist() == [1, 2, 2]


def _key(cs, pos):
    return (int(cs) << 40) | int(pos)


def test_pair_index_restatement_on_constructed_keys():
    """two cs with equal positions, a distance of exactly max_dist kept and max_dist + 1 dropped, a site without partners"""
    key = np.array([_key(0, 10), _key(0, 15), _key(0, 20), _key(0, 21), _key(0, 500), _key(1, 10), _key(1, 15)], np.int64)
    poff = P.pair_index_ref(key, 10)
    # site 0: 15 and 20 (20 - 10 == max_dist), not 21; site 1: 20, 21; site 2: 21; 21 and 500: none; cs 1: one pair, none across cs
    assert np.diff(poff).tolist() == [2, 2, 1, 0, 0, 1, 0]
    assert P.pair_index_ref(key, 11)[1] == 3 and P.pair_index_ref(key, 1).tolist() == [0, 0, 0, 1, 1, 1, 1, 1]


def test_counts_restatement_on_constructed_reads():
    """a '+' and a '-' read over three sites: the '-' read's event index runs backwards"""
    key = np.array([_key(0, 5), _key(0, 7), _key(0, 9), _key(1, 5), _key(1, 7)], np.int64)
    poff = P.pair_index_ref(key, 4)                                                          # (5, 7), (5, 9), (7, 9); (5, 7) on '-'
    assert poff.tolist() == [0, 2, 3, 3, 4, 4]
    score = np.zeros(10)
    score[[0, 2, 4]] = [3.0, -3.0, 3.0]                                                      # read 0: '+' from 5: MOD at 5, CAN at 7, MOD at 9
    score[5 + 4], score[5 + 2] = 3.0, -3.0                                                   # read 1: '-' from 3 .. 7: event 4 is pos 3 ... event 0 is pos 7
    counts = P.counts_ref(np.array([0, 1], np.int32), np.array([5, 3]), np.array([0, 5, 10]), score, key, poff, 2.5).reshape(-1, 4)
    assert counts[0].tolist() == [0, 0, 1, 0] and counts[1].tolist() == [0, 0, 0, 1] and counts[2].tolist() == [0, 1, 0, 0]
    # '-': event 0 lies at start + n - 1 = 7, event 2 at 5: pos 5 has score[5 + 2] = CAN, pos 7 has score[5 + 0] = none
    assert counts[3].tolist() == [0, 0, 0, 0]
    score[5] = 2.5                                                                           # exactly thr at pos 7: called
    counts = P.counts_ref(np.array([0, 1], np.int32), np.array([5, 3]), np.array([0, 5, 10]), score, key, poff, 2.5).reshape(-1, 4)
    assert counts[3].tolist() == [0, 1, 0, 0]


def test_header_symbols_abi_and_struct_sizes():
    text = open(HEADER).read()
    for name, val in (('MAX_DIST', L.PAIRS_MAX_DIST), ('LDS_MAX', L.PAIRS_LDS_MAX), ('THREAD_MAX', L.PAIRS_THREAD_MAX), ('FORCE_DIRECT', L.PAIRS_FORCE_DIRECT)):
        assert re.search(r'#define NMOD_PAIRS_%s (\d+)' % name, text).group(1) == str(val), name
    assert L.PAIRS_THREAD_MAX == P.THREAD_MAX and L.PAIRS_MAX_DIST <= 2 ** 20
    assert 'NMOD_PAIRS_TOO_FEW = 1, NMOD_PAIRS_DEGENERATE = 2' in text and (L.PAIRS_TOO_FEW, L.PAIRS_DEGENERATE) == (P.TOO_FEW, P.DEGENERATE) == (1, 2)
    flat = ' '.join(re.sub(r'\n \*', ' ', text).split())
    for phrase in ('int nmod_pair_index(const nmod_params* prm', 'int nmod_site_pairs(const nmod_params* prm', 'hard calls only', 'pairs only',
                   "the tie slack of R's fisher.test", 'exact as doubles while N < 2^26', 'a molecule sequenced twice'):
        assert phrase in flat, phrase
    assert re.search(r'#define NMOD_ABI_VERSION\s+4\b', text) and L.NMOD_ABI_VERSION == 4
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu", sizeof(nmod_pairs_opts), '
           'offsetof(nmod_pairs_opts, thr), sizeof(nmod_pairs_out), offsetof(nmod_pairs_out, log_or), offsetof(nmod_pairs_out, status));return 0;}' % HEADER)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == [C.sizeof(L.NmodPairsOpts), L.NmodPairsOpts.thr.offset, C.sizeof(L.NmodPairsOut), L.NmodPairsOut.log_or.offset,
                   L.NmodPairsOut.status.offset] == [24, 16, 72, 32, 64]
    lib = L.load()
    assert lib.nmod_abi_version() == 4 and lib.nmod_pair_index.argtypes is not None and lib.nmod_site_pairs.argtypes is not None


def _small_case():
    key = np.array([_key(0, 5), _key(0, 7), _key(0, 9)], np.int64)
    return dict(cs=np.array([0], np.int32), start=np.array([5], np.int64), roff=np.array([0, 5], np.int64), score=np.zeros(5), key=key,
                poff=P.pair_index_ref(key, 4))


def test_c_entries_refuse_before_any_device_work():
    """every refusal returns NMOD_ERR_INVALID_ARG (-1) with a device number that does not exist: no device was looked for"""
    lib = L.load()
    c = _small_case()
    ptr = engine._np_ptr
    npairs = C.c_int64(7)
    poff = np.zeros(4, np.int64)

    def index(prm, nsites=3, key=c['key'], max_dist=4, out=poff, n=npairs):
        return lib.nmod_pair_index(C.byref(prm) if prm is not None else None, nsites, ptr(key), max_dist, ptr(out), C.byref(n) if n is not None else None)
    host = L.make_params(device=NO_DEVICE, memspace=L.MEM_HOST)
    assert index(None) == -1 and index(L.make_params(device=NO_DEVICE, memspace=5)) == -1
    assert index(host, max_dist=0) == -1 and index(host, max_dist=L.PAIRS_MAX_DIST + 1) == -1 and index(host, nsites=-1) == -1
    assert index(host, nsites=2 ** 31 - 1) == -1 and index(host, key=None) == -1 and index(host, out=None) == -1 and index(host, n=None) == -1
    assert index(host, key=c['key'][::-1].copy()) == -1 and index(host, key=np.array([5, 5, 6], np.int64)) == -1     # host keys must strictly ascend
    assert index(host, nsites=0) == 0 and npairs.value == 0                                  # nothing to do: no device either
    assert index(host) == -5                                                                 # (a good call goes on to look for the device)

    def pairs(prm=host, nreads=1, npairs=3, opts=None, out=None, **kw):
        a = dict(c, **kw)
        opts = opts if opts is not None else L.make_pairs_opts()
        out = out if out is not None else L.make_pairs_out()
        return lib.nmod_site_pairs(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                   len(a['key']) if a['key'] is not None else 3, ptr(a['key']), ptr(a['poff']), npairs, C.byref(opts), C.byref(out))
    assert pairs(None) == -1 and pairs(nreads=2 ** 31) == -1 and pairs(nreads=-1) == -1 and pairs(npairs=2 ** 31) == -1 and pairs(npairs=-1) == -1
    for bad in (dict(thr=0.0), dict(thr=-1.0), dict(thr=float('inf')), dict(thr=float('nan')), dict(min_reads=0), dict(flags=2)):
        assert pairs(opts=L.make_pairs_opts(**bad)) == -1, bad
    short = L.make_pairs_opts(); short.struct_size -= 8
    wrong = L.make_pairs_out(); wrong.struct_size += 8
    assert pairs(opts=short) == -1 and pairs(out=wrong) == -1
    assert lib.nmod_site_pairs(C.byref(host), 1, ptr(c['cs']), ptr(c['start']), ptr(c['roff']), ptr(c['score']), 3, ptr(c['key']), ptr(c['poff']), 3,
                               None, C.byref(L.make_pairs_out())) == -1
    for missing in ('cs', 'start', 'roff', 'score', 'key', 'poff'):
        assert pairs(**{missing: None}) == -1, missing
    assert pairs(roff=np.array([5, 0], np.int64)) == -1 and pairs(key=c['key'][::-1].copy()) == -1
    assert pairs(poff=np.array([0, 3, 2, 3], np.int64)) == -1 and pairs(poff=np.array([1, 2, 3, 3], np.int64)) == -1 and pairs(npairs=2) == -1
    assert pairs(npairs=0, poff=np.zeros(4, np.int64)) == 0                                  # no pairs: nothing to do
    assert pairs() == -5


def test_python_layers_refuse_before_any_device_work():
    c = _small_case()
    args = [c[f] for f in ('cs', 'start', 'roff', 'score', 'key', 'poff')]
    for kw in (dict(thr=0.0), dict(thr=float('nan')), dict(thr=float('inf')), dict(min_reads=0), dict(min_reads=2.5), dict(want=('odds',))):
        with pytest.raises(ValueError):
            site_pairs_host(*args, device=NO_DEVICE, **kw)
    for i, bad in ((0, np.zeros(2, np.int32)), (1, np.zeros(2, np.int64)), (2, np.array([5, 0])), (4, c['key'][::-1]), (5, c['poff'][:-1]),
                   (5, np.array([0, 3, 2, 3]))):
        with pytest.raises(ValueError):
            site_pairs_host(*[bad if j == i else a for j, a in enumerate(args)], device=NO_DEVICE)
    for bad in (0, L.PAIRS_MAX_DIST + 1, 1.5):
        with pytest.raises(ValueError, match='max_dist'):
            pair_index_host(c['key'], bad, device=NO_DEVICE)
    with pytest.raises(ValueError, match='strictly ascending'):
        pair_index_host(c['key'][::-1], 4, device=NO_DEVICE)
    with pytest.raises(L.NanomodLibraryError):                                               # a good call reaches the (absent) device
        pair_index_host(c['key'], 4, device=NO_DEVICE)


def test_read_level_layer_refuses_before_any_device_work():
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    kw = dict(device=NO_DEVICE, log=lambda *a: None)
    for bad, match in ((dict(sites='all'), 'sites must be'), (dict(max_dist=0), 'max_dist'), (dict(thr=-1.0), 'thr'), (dict(min_reads=0), 'min_reads'),
                       (dict(fdr='holm'), 'fdr method'), (dict(site_alpha=0.0), 'alpha'), (dict(fdr_alpha=2.0), 'alpha'), (dict(prior=1.0), 'prior'),
                       (dict(rescale=dict(bogus=1)), 'rescale: unknown'), (dict(window=(0, 65)), 'window'),
                       (dict(sites=(np.array(['chrT']), np.array(['+']), np.array([-1]))), 'positions'),
                       (dict(sites=(np.array(['chrT']), np.array(['*']), np.array([1]))), 'strand'),
                       (dict(sites=(np.array(['chrT', 'chrT']), np.array(['+']), np.array([1]))), 'one entry per site')):
        with pytest.raises(ValueError, match=match):
            RL.cooccur_reads_llr(reads, model, alt, **dict(kw, **bad))
    per_position = dict(chrom=np.array(['chrT']), strand=np.array(['+']), pos=np.array([5]), base=np.array(['A']), off=np.array([0, 2]), sig=np.zeros(2))
    with pytest.raises(ValueError, match='not a read-level set'):
        RL.cooccur_reads_llr(per_position, model, alt, **kw)


def test_site_keys_sort_deduplicate_and_drop_unknown_chromosomes():
    got = RL.site_keys((np.array(['chrB', 'chrA', 'chrA', 'chrZ', 'chrA']), np.array(['+', '-', '+', '+', '-']), np.array([7, 3, 9, 1, 3])), ['chrA', 'chrB'])
    assert got.tolist() == [_key(0, 9), _key(1, 3), _key(2, 7)]


def test_sites_file_reader(tmp_path):
    path = str(tmp_path / 'sites.txt')
    open(path, 'w').write('# chrom strand pos\nchrT + 10 A 30 30 0.5 0.4 0.6 12.3 1.0E-03 0\n\nchrT - 11\n')
    chrom, strand, pos = RL.read_sites_file(path)
    assert chrom.tolist() == ['chrT', 'chrT'] and strand.tolist() == ['+', '-'] and pos.tolist() == [9, 10]
    for bad in ('chrT + 0\n', 'chrT * 5\n', 'chrT +\n', 'chrT + x\n'):
        open(path, 'w').write(bad)
        with pytest.raises(ValueError, match='line 1'):
            RL.read_sites_file(path)


def test_readpairs_parser_and_refusals(tmp_path, capsys):
    from nanomod_amd import cli, container
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    r = str(tmp_path / 'reads.npz')
    container.save_reads(r, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    a = cli.build_parser().parse_args(['readpairs', '--wrkBase1', r, '--kmerModel', r, '--altModel', r])
    assert (a.sites, a.maxDist, a.llrThreshold, a.llrWindow, a.prior, a.minPositions, a.rescale, a.minReads, a.siteAlpha, a.fdr, a.fdrAlpha,
            a.outFolder, a.FileID, a.device) == ('stoich', 100, 2.5, 'kmer', 0.5, 1, 0, 10, 0.05, 'none', 0.05, 'mRes', 'mod', 0)
    assert cli.validate_readpairs(a) == []
    base = ['readpairs', '--wrkBase1', r, '--kmerModel', r, '--altModel', r]
    for flag, val in (('--maxDist', '0'), ('--maxDist', str(L.PAIRS_MAX_DIST + 1)), ('--minReads', '0'), ('--siteAlpha', '0'), ('--fdrAlpha', '1.5'),
                      ('--llrThreshold', '0'), ('--llrWindow', '1,99'), ('--prior', '1'), ('--minPositions', '0')):
        assert cli.main(base + [flag, val]) == 1 and flag in capsys.readouterr().out, flag
    assert cli.main(base + ['--sites', str(tmp_path / 'none.txt')]) == 1 and 'does not exist' in capsys.readouterr().out
    g = str(tmp_path / 'group.npz')
    np.savez(g, chrom=np.array(['chrT']), strand=np.array(['+']), pos=np.array([5]), base=np.array(['A']), off=np.array([0, 2]), sig=np.zeros(2))
    assert cli.main(['readpairs', '--wrkBase1', g, '--kmerModel', r, '--altModel', r]) == 1 and 'not a read-level container' in capsys.readouterr().out


def test_write_site_pairs_format(tmp_path):
    nan = np.nan
    pairs = dict(chrom=np.array(['chrT', 'chrT']), strand=np.array(['+', '-']), pos_a=np.array([9, 10]), pos_b=np.array([19, 40]), dist=np.array([10, 30]),
                 n11=np.array([30, 1], np.int32), n10=np.array([2, 0], np.int32), n01=np.array([3, 0], np.int32), n00=np.array([31, 1], np.int32),
                 log_or=np.array([4.5, nan]), se=np.array([0.25, nan]), phi=np.array([-0.5, nan]), p_fisher=np.array([4.4e-14, nan]),
                 status=np.array([0, 1], np.uint8))
    path = str(tmp_path / 'run_site_pairs.txt')
    RL.write_site_pairs(path, pairs)
    assert open(path).read() == ('chrT + 10 20 10 30 2 3 31 4.500000 0.250000 -0.500000 4.400E-14 0\n'
                                 'chrT - 11 41 30 1 0 0 1 nan nan nan nan 1\n')
    RL.write_site_pairs(path, dict(pairs, q=np.array([8.8e-14, nan])))
    lines = open(path).read().splitlines()
    assert lines[0].endswith(' 4.400E-14 8.800E-14 0') and lines[1].endswith(' nan nan 1')
