"""nmod_pair_rows_count / nmod_pair_rows_fill / nmod_pair_linkage (K18) without a GPU: the restatement of the header's definition
(tests/linkage_ref.py) — its stage 1 against stoich_ref, a closed form on perfect calls, the two-stage statistic against the full
four-weight model by EM, the null level of p_indep —, the rows on a constructed case, the declarations and struct layouts, and the
refusals of every layer before any device work.

Measured with the seeds below (4 000 null pairs each, rejected at the 5 % level): 0.053 at 200 reads, 3 sd, shares 0.3 / 0.5 (the
calibration cell: it must lie within 0.05 +- 0.015, about four binomial standard errors); 0.057 at 20 reads, 3 sd, 0.5 / 0.5; 0.068 at
10 reads, 3 sd, 0.5 / 0.5; 0.032 at 200 reads, 1 sd, 0.3 / 0.3; 0.024 at 200 reads, 3 sd, 0.05 / 0.05.  With D = 0.1 at 2 sd, shares
0.3 / 0.3, 100 reads: 0.70 of 1 000 pairs rejected."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import linkage_ref as K
import pairs_ref as P
import stoich_ref as F
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL
from nanomod_amd.engine import pair_linkage_host, pair_rows_host             # K18's entries: without them nothing here can pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
NO_DEVICE = 10 ** 6                                                           # a device that does not exist: a call that reaches it fails


def _key(cs, pos):
    return (int(cs) << 40) | int(pos)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_stage_one_is_stoich_ref_on_the_same_row():
    rng = np.random.default_rng(1820)
    for sep, pa, pb, d in ((3.0, 0.3, 0.5, 0.05), (1.5, 0.2, 0.2, 0.0), (2.0, 0.5, 0.5, -0.1)):
        sa, sb = K.simulate_pair(rng, 80, sep, pa, pb, d)
        r = K.row(sa, sb)
        assert r['pa'] == F.row(sa, min_valid=1)['pi'] and r['pb'] == F.row(sb, min_valid=1)['pi'] and not r['status'] & ~(K.AT_MIN | K.AT_MAX)
        # a read that is invalid on one side leaves both rows
        sa2, sb2 = sa.copy(), sb.copy()
        sa2[3], sb2[10] = np.nan, np.inf
        keep = np.ones(80, bool)
        keep[[3, 10]] = False
        r2 = K.row(sa2, sb2)
        assert r2['n_valid'] == 78 and r2['pa'] == F.row(sa[keep], min_valid=1)['pi'] and r2['pb'] == F.row(sb[keep], min_valid=1)['pi']
        assert r2['d'] == K.row(sa[keep], sb[keep])['d']


def test_perfect_calls_give_the_table_s_closed_form():
    """|s| = 40: t rounds to 1, every read is a call.  D^ = n11 / n - (r1 / n)(c1 / n), and stat is the G statistic of the 2 x 2 table"""
    rng = np.random.default_rng(1821)
    for n, pa, pb, d in ((80, 0.4, 0.5, 0.1), (200, 0.3, 0.3, -0.03), (50, 0.5, 0.6, 0.0)):
        p11, p10, p01, p00 = K.cells(pa, pb, d)
        state = rng.choice(4, size=n, p=[p00, p01, p10, p11])
        za, zb = state >= 2, (state & 1) == 1
        r = K.row(np.where(za, 40.0, -40.0), np.where(zb, 40.0, -40.0), tol=1e-14)
        tab = np.array([[(za & zb).sum(), (za & ~zb).sum()], [(~za & zb).sum(), (~za & ~zb).sum()]], float)
        assert tab.min() > 0 and r['status'] == 0
        want_d = tab[0, 0] / n - (tab[0].sum() / n) * (tab[:, 0].sum() / n)
        expected = np.outer(tab.sum(1), tab.sum(0)) / n
        g_stat = 2.0 * float((tab * np.log(tab / expected)).sum())
        assert abs(r['pa'] - tab[0].sum() / n) < 1e-12 and abs(r['pb'] - tab[:, 0].sum() / n) < 1e-12
        assert abs(r['d'] - want_d) < 1e-12 and abs(r['stat'] - g_stat) < 1e-9 * max(1.0, g_stat), (r['d'], want_d, r['stat'], g_stat)
        assert r['d_lo'] < r['d'] < r['d_hi'] and abs(r['r'] - want_d / math.sqrt(r['pa'] * (1 - r['pa']) * r['pb'] * (1 - r['pb']))) < 1e-10
    # perfectly linked and perfectly exclusive calls sit at the ends of the range
    s = np.where(rng.random(60) < 0.4, 40.0, -40.0)
    hi, lo = K.row(s, s), K.row(s, -s)
    assert hi['status'] == K.AT_MAX and lo['status'] == K.AT_MIN and hi['iters'] == lo['iters'] == 0
    assert hi['d'] == hi['d_hi'] > hi['d_lo'] > 0.0 and lo['d'] == lo['d_lo'] < lo['d_hi'] < 0.0 and abs(hi['r'] - 1.0) < 1e-12 and abs(lo['r'] + 1.0) < 1e-12


def test_the_statistic_never_exceeds_the_full_model_s():
    """60 seeded pairs at 2 and 3 sd: stat <= the full four-weight likelihood-ratio statistic (EM from the independence table) + 1e-6"""
    rng = np.random.default_rng(1822)
    ratios = []
    for i in range(60):
        sep, n = (3.0, 2.0)[i % 2], (50, 100, 200)[i % 3]
        sa, sb = K.simulate_pair(rng, n, sep, (0.3, 0.5)[i % 2], (0.4, 0.3, 0.5)[i % 3], (0.0, 0.1, -0.05, 0.0)[i % 4])
        r = K.row(sa, sb)
        full, converged = K.full_stat(sa, sb)
        assert r['stat'] <= full + 1e-6, (i, r['stat'], full, converged)
        if full > 1.0:
            ratios.append(r['stat'] / full)
    print('two-stage / full statistic over %d pairs: median %.4f, least %.4f' % (len(ratios), float(np.median(ratios)), min(ratios)))
    assert np.median(ratios) > 0.9


def test_p_indep_holds_its_level_on_null_pairs():
    share = K.null_share(200, 3.0, 0.3, 0.5, 1810)
    print('4 000 null pairs, 200 reads, 3 sd, shares 0.3 / 0.5: %.4f rejected at the 5 %% level' % share)
    assert abs(share - 0.05) <= 0.015
    low = K.null_share(20, 3.0, 0.5, 0.5, 1811)
    print('4 000 null pairs, 20 reads, 3 sd, shares 0.5 / 0.5: %.4f rejected at the 5 %% level' % low)
    flat = ' '.join(re.sub(r'\n \*', ' ', open(HEADER).read()).split())
    assert '%.3f at 200 reads, 3 sd, shares 0.3 / 0.5' % share in flat and '%.3f at 20 reads, 3 sd, 0.5 / 0.5' % low in flat   # the header's record
    # the batch estimate is the definition's statistic
    rng = np.random.default_rng(1823)
    for _ in range(5):
        sa, sb = K.simulate_pair(rng, 60, 2.0, 0.3, 0.4, 0.05)
        assert abs(K.stat_batch(sa[None], sb[None])[0] - K.row(sa, sb)['stat']) < 1e-8


def test_the_liberal_and_the_conservative_corners_are_reported():
    """the cells the header names beside the calibration cell: measured, printed, and the header's record of them"""
    flat = ' '.join(re.sub(r'\n \*', ' ', open(HEADER).read()).split())
    for n, sep, pa, pb, seed, text in ((10, 3.0, 0.5, 0.5, 1812, '%.3f at 10 reads, 3 sd, 0.5 / 0.5'), (200, 1.0, 0.3, 0.3, 1813, '%.3f at 200 reads, 1 sd, 0.3 / 0.3'),
                                       (200, 3.0, 0.05, 0.05, 1814, '%.3f at 200 reads, 3 sd, 0.05 / 0.05')):
        share = K.null_share(n, sep, pa, pb, seed)
        print('4 000 null pairs, %d reads, %g sd, shares %g / %g: %.4f rejected at the 5 %% level' % (n, sep, pa, pb, share))
        assert text % share in flat, text % share
    power = K.null_share(100, 2.0, 0.3, 0.3, 1815, N=1000, d=0.1)
    print('1 000 pairs of 100 reads, 2 sd, shares 0.3 / 0.3, D = 0.1: %.3f rejected at the 5 %% level' % power)
    assert power > 0.32                                                                  # K16's exact test on the called reads of such pairs, in the simulation behind K18: the soft test must do better


def test_statuses_of_the_planted_rows():
    sa, sb, off, names = K.planted_batch()
    st = dict(zip(names, K.expected('planted')))
    assert st['too_few']['status'] == st['invalid_mix']['status'] == K.TOO_FEW and st['invalid_mix']['n_valid'] == 19
    assert st['flat_a']['status'] == st['flat_b']['status'] == K.FLAT and np.isnan(st['flat_a']['d'])
    for name in ('degenerate_a0', 'degenerate_b1'):
        e = st[name]
        assert (e['status'], e['d'], e['d_lo'], e['d_hi'], e['stat'], e['p_indep'], e['iters']) == (K.DEGENERATE, 0.0, 0.0, 0.0, 0.0, 1.0, 0) and np.isnan(e['r'])
    assert st['degenerate_a0']['pa'] == 0.0 and st['degenerate_b1']['pb'] == 1.0
    assert K.row(np.zeros(5), np.zeros(5), min_reads=1)['status'] == K.FLAT and K.row(np.zeros(0), np.zeros(0))['status'] == K.TOO_FEW
    e = K.row(sa[:60], sb[:60], max_iter=1)
    assert e['status'] == K.NOT_CONVERGED and e['iters'] == 1
    p11, p10, p01, p00 = K.cells(0.3, 0.4, 0.05)
    assert abs(p11 + p10 - 0.3) < 1e-15 and abs(p11 + p01 - 0.4) < 1e-15 and abs(p11 + p10 + p01 + p00 - 1.0) < 1e-15


def test_rows_restatement_on_constructed_reads():
    """a '+' and a '-' read over three sites: the '-' read's event index runs backwards; an invalid score drops the read from a pair"""
    key = np.array([_key(0, 5), _key(0, 7), _key(0, 9), _key(1, 5), _key(1, 7)], np.int64)
    poff = P.pair_index_ref(key, 4)                                                          # (5, 7), (5, 9), (7, 9); (5, 7) on '-'
    score = np.zeros(15)
    score[[0, 2, 4]] = [1.0, np.nan, -2.0]                                                   # read 0: '+' from 5: 1.0 at 5, NaN at 7, -2.0 at 9
    score[5 + 4], score[5 + 2], score[5 + 0] = 9.0, 0.5, -0.25                               # read 1: '-' from 3 .. 7: event 2 is pos 5, event 0 pos 7
    score[10:15] = [3.0, 0.0, -3.0, 0.0, np.inf]                                             # read 2: '+' from 5: 3.0, -3.0, inf at 9
    rows = K.pair_rows_ref(np.array([0, 1, 0], np.int32), np.array([5, 3, 5]), np.array([0, 5, 10, 15]), score, key, poff)
    assert rows['prow_off'].tolist() == [0, 1, 2, 2, 3]
    assert rows['read'].tolist() == [2, 0, 1] and rows['sa'].tolist() == [3.0, 1.0, 0.5] and rows['sb'].tolist() == [-3.0, -2.0, -0.25]


# ------------------------------------------------------------------------------------------------------------ the declarations
def test_header_symbols_abi_and_struct_sizes():
    text = open(HEADER).read()
    for name, val in (('SMALL', L.LINK_SMALL), ('WAVE', L.LINK_WAVE)):
        assert re.search(r'#define NMOD_LINK_%s (\d+)' % name, text).group(1) == str(val), name
    assert (L.LINK_SMALL, L.LINK_WAVE) == (L.STOICH_SMALL, L.STOICH_WAVE) == (K.SMALL, K.WAVE)
    assert ('NMOD_LINK_TOO_FEW = 1, NMOD_LINK_FLAT = 2, NMOD_LINK_NOT_CONVERGED = 4, NMOD_LINK_AT_MIN = 8, NMOD_LINK_AT_MAX = 16,\n'
            '       NMOD_LINK_TOO_LARGE = 32, NMOD_LINK_DEGENERATE = 64') in text
    assert (L.LINK_TOO_FEW, L.LINK_FLAT, L.LINK_NOT_CONVERGED, L.LINK_AT_MIN, L.LINK_AT_MAX, L.LINK_TOO_LARGE, L.LINK_DEGENERATE) == \
           (K.TOO_FEW, K.FLAT, K.NOT_CONVERGED, K.AT_MIN, K.AT_MAX, K.TOO_LARGE, K.DEGENERATE)
    assert L.LINK_FIELDS == K.FIELDS
    flat = ' '.join(re.sub(r'\n \*', ' ', text).split())
    for phrase in ('int nmod_pair_rows_count(const nmod_params* prm', 'int nmod_pair_rows_fill(const nmod_params* prm',
                   'int nmod_pair_linkage(const nmod_params* prm', 'A TWO-STAGE estimate', 'information-orthogonal', 'IN ASCENDING READ INDEX',
                   'never exceeds the full likelihood-ratio statistic', 'no interval for the pi cells', 'p_indep is unadjusted'):
        assert phrase in flat, phrase
    assert re.search(r'#define NMOD_ABI_VERSION\s+4\b', text) and L.NMOD_ABI_VERSION == 4      # purely additive entries
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu", sizeof(nmod_link_opts), '
           'offsetof(nmod_link_opts, tol), sizeof(nmod_link_out), offsetof(nmod_link_out, pa), offsetof(nmod_link_out, n_valid), '
           'offsetof(nmod_link_out, status));return 0;}' % HEADER)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == [C.sizeof(L.NmodLinkOpts), L.NmodLinkOpts.tol.offset, C.sizeof(L.NmodLinkOut), L.NmodLinkOut.pa.offset, L.NmodLinkOut.n_valid.offset,
                   L.NmodLinkOut.status.offset] == [32, 16, 96, 8, 72, 88]
    lib = L.load()
    for name in ('nmod_pair_rows_count', 'nmod_pair_rows_fill', 'nmod_pair_linkage'):
        assert name in L._SIGNATURES and getattr(lib, name).argtypes is not None
    src = open(os.path.join(ROOT, 'nanomod_amd', 'csrc', 'site_linkage.hip')).read()
    assert '#include "stoich_rows.hpp"' in src and 'st_solve<0>' in src and 'atomic' not in src.split('#include', 1)[1]      # K14's functions; no atomics
    mk = open(os.path.join(ROOT, 'nanomod_amd', 'csrc', 'Makefile')).read()      # contraction off for the unit: its target-specific flag, used by the one .hip rule
    assert re.search(r'^\$\(OBJDIR\)/site_linkage\.o: CXXFLAGS \+= -ffp-contract=off$', mk, re.M)
    assert re.search(r'^\$\(OBJDIR\)/%\.o: %\.hip .*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -c', mk, re.M) and 'site_linkage.o' in re.search(r'^OBJS\s*=((?:.*\\\n)*.*)$', mk, re.M).group(1)


def _small_case():
    key = np.array([_key(0, 5), _key(0, 7), _key(0, 9)], np.int64)
    return dict(cs=np.array([0], np.int32), start=np.array([5], np.int64), roff=np.array([0, 5], np.int64), score=np.zeros(5), key=key,
                poff=P.pair_index_ref(key, 4))


def test_c_entries_refuse_before_any_device_work():
    """every refusal returns NMOD_ERR_INVALID_ARG (-1) with a device number that does not exist: no device was looked for"""
    lib = L.load()
    c = _small_case()
    ptr = engine._np_ptr
    host = L.make_params(device=NO_DEVICE, memspace=L.MEM_HOST)
    prow = np.zeros(4, np.int64)
    nrows = C.c_int64(7)

    def count(prm=host, nreads=1, npairs=3, out=prow, n=nrows, **kw):
        a = dict(c, **kw)
        return lib.nmod_pair_rows_count(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                        len(a['key']) if a['key'] is not None else 3, ptr(a['key']), ptr(a['poff']), npairs, ptr(out),
                                        C.byref(n) if n is not None else None)
    assert count(None) == -1 and count(L.make_params(device=NO_DEVICE, memspace=5)) == -1 and count(nreads=2 ** 31) == -1 and count(npairs=-1) == -1
    assert count(out=None) == -1 and count(n=None) == -1 and count(npairs=2) == -1
    for missing in ('cs', 'start', 'roff', 'score', 'key', 'poff'):
        assert count(**{missing: None}) == -1, missing
    assert count(roff=np.array([5, 0], np.int64)) == -1 and count(key=c['key'][::-1].copy()) == -1 and count(poff=np.array([0, 3, 2, 3], np.int64)) == -1
    assert count(npairs=0, poff=np.zeros(4, np.int64)) == 0 and nrows.value == 0           # no pairs: nothing to do, no device either
    assert count() == -5                                                                     # (a good call goes on to look for the device)

    sa, sb, rd = np.zeros(2), np.zeros(2), np.zeros(2, np.int32)
    good = np.array([0, 1, 2, 2], np.int64)

    def fill(prm=host, nreads=1, npairs=3, prow_off=good, n=2, **kw):
        a = dict(c, **kw)
        return lib.nmod_pair_rows_fill(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                       len(a['key']), ptr(a['key']), ptr(a['poff']), npairs, ptr(prow_off), n, ptr(sa), ptr(sb), ptr(rd))
    assert fill(None) == -1 and fill(n=-1) == -1 and fill(n=2 ** 31) == -1 and fill(prow_off=None) == -1 and fill(n=3) == -1
    assert fill(prow_off=np.array([1, 1, 2, 2], np.int64)) == -1 and fill(prow_off=np.array([0, 2, 1, 2], np.int64)) == -1
    assert fill(key=c['key'][::-1].copy()) == -1 and fill(cs=None) == -1 and fill(nreads=0, roff=np.array([0], np.int64)) == -1
    assert fill(prow_off=np.zeros(4, np.int64), n=0) == 0                                   # no rows: nothing to do
    assert fill() == -5

    off = np.array([0, 2], np.int64)

    def link(prm=host, npairs=1, a=sa, b=sb, o=off, opts=None, out=None):
        opts = opts if opts is not None else L.make_link_opts()
        out = out if out is not None else L.make_link_out()
        return lib.nmod_pair_linkage(C.byref(prm) if prm is not None else None, npairs, ptr(a), ptr(b), ptr(o), C.byref(opts), C.byref(out))
    assert link(None) == -1 and link(npairs=-1) == -1 and link(npairs=2 ** 31 - 1) == -1 and link(o=None) == -1 and link(a=None) == -1 and link(b=None) == -1
    for bad in (dict(max_iter=0), dict(max_iter=201), dict(min_reads=0), dict(tol=-1.0), dict(tol=float('nan')), dict(tol=float('inf')),
                dict(ci_drop=0.0), dict(ci_drop=float('inf')), dict(ci_drop=float('nan'))):
        assert link(opts=L.make_link_opts(**bad)) == -1, bad
    short = L.make_link_opts(); short.struct_size -= 8
    wrong = L.make_link_out(); wrong.struct_size += 8
    assert link(opts=short) == -1 and link(out=wrong) == -1 and link(o=np.array([2, 0], np.int64)) == -1
    assert lib.nmod_pair_linkage(C.byref(host), 1, ptr(sa), ptr(sb), ptr(off), None, C.byref(L.make_link_out())) == -1
    assert link(npairs=0) == 0 and link() == -5
    assert link(a=None, b=None, o=np.zeros(2, np.int64)) == -5                               # host rows that are all empty need no scores


def test_python_layers_refuse_before_any_device_work():
    c = _small_case()
    args = [c[f] for f in ('cs', 'start', 'roff', 'score', 'key', 'poff')]
    for i, bad in ((0, np.zeros(2, np.int32)), (1, np.zeros(2, np.int64)), (2, np.array([5, 0])), (4, c['key'][::-1]), (5, c['poff'][:-1]),
                   (5, np.array([0, 3, 2, 3]))):
        with pytest.raises(ValueError):
            pair_rows_host(*[bad if j == i else a for j, a in enumerate(args)], device=NO_DEVICE)
    with pytest.raises(L.NanomodLibraryError):                                               # a good call reaches the (absent) device
        pair_rows_host(*args, device=NO_DEVICE)
    sa, sb, off = np.zeros(4), np.zeros(4), np.array([0, 2, 4])
    for kw in (dict(min_reads=0), dict(min_reads=2.5), dict(ci_level=0.0), dict(ci_level=1.0), dict(max_iter=0), dict(max_iter=201), dict(tol=-1.0),
               dict(tol=float('nan'))):
        with pytest.raises(ValueError):
            pair_linkage_host(sa, sb, off, device=NO_DEVICE, **kw)
    for bad in ((sa, sb[:3], off), (sa, sb, np.array([0, 5])), (sa, sb, np.array([0, 3, 2])), (sa.reshape(2, 2), sb.reshape(2, 2), off)):
        with pytest.raises(ValueError):
            pair_linkage_host(*bad, device=NO_DEVICE)
    with pytest.raises(L.NanomodLibraryError):
        pair_linkage_host(sa, sb, off, device=NO_DEVICE)
    o = engine._link_opts(20, 0.95, 60, 1e-12)
    assert (o.min_reads, o.max_iter, o.tol) == (20, 60, 1e-12) and abs(o.ci_drop - F.CI_DROP_95) < 1e-12
    assert set(engine._link_shapes(3, interval=False)) == set(L.LINK_FIELDS + L.LINK_INT_FIELDS + ('status',)) - {'d_lo', 'd_hi'}


def test_read_level_layer_and_command_line_refuse_before_any_device_work(tmp_path, capsys):
    import readllr_ref as RF
    from nanomod_amd import cli, container
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    for bad in (0.0, 1.0, -0.5):
        with pytest.raises(ValueError, match='ci_level'):
            RL.cooccur_reads_llr(reads, model, alt, soft=True, ci_level=bad, device=NO_DEVICE, log=lambda *a: None)
    r = str(tmp_path / 'reads.npz')
    container.save_reads(r, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    base = ['readpairs', '--wrkBase1', r, '--kmerModel', r, '--altModel', r]
    a = cli.build_parser().parse_args(base)
    assert (a.soft, a.ciLevel) == (0, 0.95) and cli.validate_readpairs(a) == []            # off by default
    assert cli.main(base + ['--soft', '1', '--ciLevel', '1']) == 1 and '--ciLevel' in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ['--soft', '2'])


def test_write_site_linkage_format(tmp_path):
    nan = np.nan
    pairs = dict(chrom=np.array(['chrT', 'chrT']), strand=np.array(['+', '-']), pos_a=np.array([9, 10]), pos_b=np.array([19, 40]), dist=np.array([10, 30]),
                 n_cov=np.array([80, 5], np.int32), pa=np.array([0.5, nan]), pb=np.array([0.25, nan]), d=np.array([0.1, nan]), d_lo=np.array([0.05, nan]),
                 d_hi=np.array([0.125, nan]), r=np.array([0.4618802, nan]), pi11=np.array([0.225, nan]), pi10=np.array([0.275, nan]),
                 pi01=np.array([0.025, nan]), pi00=np.array([0.475, nan]), stat=np.array([17.25, nan]), p_indep=np.array([3.3e-5, nan]),
                 link_status=np.array([0, 1], np.uint8))
    path = str(tmp_path / 'run_site_linkage.txt')
    RL.write_site_linkage(path, pairs)
    assert open(path).read() == ('chrT + 10 20 10 80 0.500000 0.250000 0.100000 0.050000 0.125000 0.461880 0.225000 0.275000 0.025000 0.475000 17.250 3.300E-05 0\n'
                                 'chrT - 11 41 30 5 nan nan nan nan nan nan nan nan nan nan nan nan 1\n')
    RL.write_site_linkage(path, dict(pairs, q_indep=np.array([6.6e-5, nan])))
    lines = open(path).read().splitlines()
    assert lines[0].endswith('3.300E-05 6.600E-05 0') and lines[1].endswith('nan nan 1')
