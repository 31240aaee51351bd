"""nmod_site_diff (K15) without a GPU: the numpy restatement of the header's definition (tests/diff_ref.py) against 50-digit mpmath
within the gates it derives, known answers, the null level of p_diff by a vectorised estimate of the definition, the declarations
and struct layouts, and the refusals of the Python layers before any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import diff_ref as F
import stoich_ref as SR
import readllr_ref as RF
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL
from nanomod_amd.engine import site_diff_host             # K15's entry: without it nothing here can pass

PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'site_diff.txt')
_erfc = np.vectorize(math.erfc, otypes=[np.float64])
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nanomod_hip.h')


def _share(name, dev, gate, worst):
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0: %r' % (name, dev)
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def test_restatement_is_pinned_against_mpmath():
    """14 seeded pairs of rows (3 .. 30 reads, separations 0.3 .. 8 sd, equal and unequal shares 0 .. 1) and constructed ones: every
    output within its gate of the 50-digit solution, exactly equal at an end of [0, 1] or of [-1, 1]"""
    rng = np.random.default_rng(1503)
    pairs = []
    for k in range(14):
        sep = SR.SEPARATIONS[k % 4]
        p0, p1 = ((0.3, 0.3), (0.1, 0.8), (0.0, 0.6), (1.0, 0.4), (0.5, 0.5), (0.0, 0.0), (0.9, 1.0))[k % 7]
        pairs.append((SR.simulate_row(rng, int(rng.choice([3, 8, 30])), sep, p0), SR.simulate_row(rng, int(rng.choice([4, 12, 30])), sep, p1)))
    pairs += [(np.array([800.0, 800.0, 800.0, -800.0]), np.array([800.0, -800.0, -800.0, -800.0])),
              (np.array([-800.0] * 5), np.array([800.0] * 5)), (np.array([np.nan, 2.0, -1.0, np.inf, 0.7]), np.array([0.0, -0.0, 1.0, -2.0, 0.5]))]
    worst, ends = {}, 0
    for s0, s1 in pairs:
        r, x = F.site(s0, s1, min_valid=1), F.exact_site(s0, s1)
        assert r['status'] & ~F.POOL_AT_END == 0, r
        for f in ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat'):
            _share(f, abs(float(x[f] - r[f])), r['gates'][f], worst)
        lo, hi = r['gates']['p_diff']
        assert lo <= float(x['p_diff']) <= hi, (lo, float(x['p_diff']), hi)
        ends += r['delta_lo'] == -1.0 or r['delta_hi'] == 1.0
    print('worst deviation as a share of its gate: %s; %d of %d pairs with an interval end at +-1'
          % (', '.join('%s %.3g' % kv for kv in sorted(worst.items())), ends, len(pairs)))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_known_answers():
    a, b = np.array([800.0, 800.0, 800.0, -800.0]), np.array([800.0, -800.0, -800.0, -800.0])
    r = F.site(a, b)
    # the likelihoods are p^3 (1 - p) and p (1 - p)^3: shares 3/4 and 1/4, pooled 1/2
    assert abs(r['pi0'] - 0.75) <= r['gates']['pi0'] and abs(r['pi1'] - 0.25) <= r['gates']['pi1'] and abs(r['pi_pool'] - 0.5) <= r['gates']['pi_pool']
    assert abs(r['delta'] + 0.5) <= r['gates']['delta'] and r['status'] == 0 and (r['n_valid0'], r['n_valid1']) == (4, 4) and 0 < r['iters'] <= 60
    ll = lambda p: 3.0 * math.log(p) + math.log(1.0 - p)
    assert abs(r['stat'] - 4.0 * (ll(0.75) - ll(0.5))) < 1e-9
    assert abs(r['p_diff'] - math.erfc(math.sqrt(r['stat'] / 2.0))) < 1e-15
    assert -1.0 < r['delta_lo'] < -0.5 < r['delta_hi'] < 1.0
    # the same row twice: nothing differs
    r = F.site(a, a)
    assert r['pi0'] == r['pi1'] and r['delta'] == 0.0 and r['stat'] <= r['gates']['stat'] and r['delta_lo'] < 0.0 < r['delta_hi']
    # all canonical against all modified: delta = 1, the pooled share inside, the interval ends at 1
    r = F.site(np.array([-800.0] * 5), np.array([800.0] * 5))
    assert (r['pi0'], r['pi1'], r['delta'], r['delta_hi'], r['status']) == (0.0, 1.0, 1.0, 1.0, 0) and abs(r['pi_pool'] - 0.5) < 1e-9
    assert 0.0 < r['delta_lo'] < 1.0
    # both canonical: the pooled share is 0 too
    r = F.site(np.array([-3.0, -1.0, -800.0]), np.array([-2.0, -0.5, -4.0]))
    assert (r['pi0'], r['pi1'], r['pi_pool'], r['delta'], r['stat'], r['p_diff'], r['iters'], r['status']) == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0, F.POOL_AT_END)
    assert r['delta_lo'] < 0.0 < r['delta_hi']
    r = F.site(np.array([1.0, np.nan, -1.0]), a)
    assert r['status'] == F.TOO_FEW and (r['n_valid0'], r['n_valid1']) == (2, 4) and all(np.isnan(r[f]) for f in F.FIELDS) and r['iters'] == 0
    r = F.site(a, np.array([0.0, -0.0, 0.0]))
    assert r['status'] == F.FLAT and (r['n_valid0'], r['n_valid1']) == (4, 3) and np.isnan(r['stat'])
    r = F.site(np.array([2.0, -1.0, 0.5, -0.3]), np.array([1.0, -2.0, 0.1]), max_iter=1)
    assert r['status'] & F.NOT_CONVERGED and r['iters'] == 1


def test_the_test_and_the_interval_are_one_statement():
    """stat is the profile deviance at 0: above ci_drop by more than the gate, 0 lies outside [delta_lo, delta_hi]; below, inside"""
    rng = np.random.default_rng(1504)
    seen = [0, 0]
    for k in range(24):
        p1 = (0.3, 0.45, 0.6, 0.9)[k % 4]
        r = F.site(SR.simulate_row(rng, 30, 3.0, 0.3), SR.simulate_row(rng, 30, 3.0, p1))
        if r['gates'] is None:
            continue
        if r['stat'] > SR.DEFAULTS['ci_drop'] + r['gates']['stat']:
            seen[0] += 1
            assert not r['delta_lo'] <= 0.0 <= r['delta_hi'], r
        elif r['stat'] < SR.DEFAULTS['ci_drop'] - r['gates']['stat']:
            seen[1] += 1
            assert r['delta_lo'] <= 0.0 <= r['delta_hi'], r
    assert min(seen) >= 4, seen


def _null_share(n, sep, pi, seed, N=40000):
    """the share of N null pairs (n v n reads, levels sep sd apart, a share pi modified in both) with p_diff <= 0.05, by the
    definition's estimates found by 32 vectorised halvings of the score per row (a property of the definition, not of the kernels)"""
    rng = np.random.default_rng(seed)

    def sim(rows):
        z = rng.random((rows, n)) < pi
        return sep * (rng.normal(size=(rows, n)) + sep * z) - 0.5 * sep * sep

    def mle(s):
        t = -np.expm1(-np.abs(s)) * np.where(s >= 0.0, 1.0, -1.0)
        ta, plus = np.abs(t), t >= 0.0

        def S(p):
            with np.errstate(divide='ignore', invalid='ignore'):
                u = ta / (1.0 - np.where(plus, 1.0 - p[:, None], p[:, None]) * ta)
            return np.where(plus, u, -u).sum(1)

        def g(p):
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.log1p(-np.where(plus, 1.0 - p[:, None], p[:, None]) * ta).sum(1)
        lo, hi = np.zeros(len(s)), np.ones(len(s))
        at0 = S(lo) <= 0.0
        at1 = ~at0 & (S(hi) >= 0.0)
        for _ in range(32):
            m = 0.5 * (lo + hi)
            r = S(m) > 0.0
            lo, hi = np.where(r, m, lo), np.where(r, hi, m)
        p = np.where(at0, 0.0, np.where(at1, 1.0, 0.5 * (lo + hi)))
        return p, g(p)
    rej, done = 0, 0
    while done < N:
        rows = min(10000, N - done)
        a, b = sim(rows), sim(rows)
        (_, ga), (_, gb) = mle(a), mle(b)
        _, gpool = mle(np.concatenate([a, b], 1))
        stat = np.maximum(2.0 * (ga + gb - gpool), 0.0)
        rej += int((np.maximum(_erfc(np.sqrt(0.5 * stat)), SR.DBL_MIN) <= 0.05).sum())
        done += rows
    return rej / N


@pytest.mark.parametrize('n, sep, pi', [(20, 1.0, 0.3), (200, 1.0, 0.3), (200, 3.0, 0.5), (20, 3.0, 0.5)])
def test_p_diff_holds_its_level_on_null_pairs(n, sep, pi):
    """40 000 seeded null pairs: the share with p_diff <= 0.05 may not exceed 0.0603, the project's bound from K14's level test"""
    share = _null_share(n, sep, pi, 1510 + n + int(10 * sep))
    print('null pairs %d v %d, sep %g, pi %g: %.4f rejected at the 5 %% level' % (n, n, sep, pi, share))
    assert share <= 0.0603


@pytest.mark.parametrize('pi', [0.0, 1.0])
def test_p_diff_is_conservative_at_the_ends(pi):
    share = _null_share(20, 3.0, pi, 1530 + int(pi))
    print('null pairs 20 v 20, sep 3, pi %g: %.4f rejected at the 5 %% level' % (pi, share))
    assert share <= 0.05


def _recorded(n, sep, pi):
    """the share profiles/site_diff.txt records for a configuration"""
    m = re.search(r'^\s+%d v %d\s+%g\s+%g\s+(0\.\d{4})\b' % (n, n, sep, pi), open(PROFILE).read(), re.M)
    assert m, 'profiles/site_diff.txt has no row for %d v %d, sep %g, pi %g' % (n, n, sep, pi)
    return float(m.group(1))


def test_the_liberal_corners_are_reported():
    """10 v 10 and 200 v 200 at a share of 0.02: printed, not bounded (the header names the law as slightly liberal at low coverage); the
    profile file records these very figures"""
    for n, sep, pi in ((10, 3.0, 0.5), (200, 3.0, 0.02)):
        share = _null_share(n, sep, pi, 1540 + n)
        print('null pairs %d v %d, sep %g, pi %g: %.4f rejected at the 5 %% level' % (n, n, sep, pi, share))
        assert '%.4f' % share == '%.4f' % _recorded(n, sep, pi)


def test_header_symbol_and_abi():
    text = open(HEADER).read()
    assert re.search(r'#define NMOD_DIFF_SMALL (\d+)', text).group(1) == str(F.SMALL) == str(L.DIFF_SMALL)
    assert re.search(r'#define NMOD_DIFF_WAVE (\d+)', text).group(1) == str(F.WAVE) == str(L.DIFF_WAVE)
    assert 'NMOD_DIFF_TOO_FEW = 1, NMOD_DIFF_FLAT = 2, NMOD_DIFF_NOT_CONVERGED = 4, NMOD_DIFF_POOL_AT_END = 8, NMOD_DIFF_TOO_LARGE = 32' in text
    assert (L.DIFF_TOO_FEW, L.DIFF_FLAT, L.DIFF_NOT_CONVERGED, L.DIFF_POOL_AT_END, L.DIFF_TOO_LARGE) == (1, 2, 4, 8, 32) == \
        (F.TOO_FEW, F.FLAT, F.NOT_CONVERGED, F.POOL_AT_END, F.TOO_LARGE)
    for phrase in ('int nmod_site_diff(const nmod_params* prm', 'treated as independent', 'each strand is its own site', 'asymptotic',
                   'both k-mer tables are taken as', 'iters = the evaluations the iteration for pi_pool made'):
        assert phrase in text, phrase
    assert re.search(r'#define NMOD_ABI_VERSION\s+4\b', text) and L.NMOD_ABI_VERSION == 4
    assert C.sizeof(L.NmodDiffOpts) == 32 and C.sizeof(L.NmodDiffOut) == 8 + 12 * 8
    assert L.DIFF_FIELDS == F.FIELDS
    lib = L.load()
    assert lib.nmod_abi_version() == 4 and lib.nmod_site_diff.argtypes is not None


def test_refusals_before_any_device_work():
    a = np.array([1.0, -1.0, 2.0, 0.5])
    off = np.array([0, 4], np.int64)
    for kw in (dict(ci_level=1.0), dict(ci_level=0.0), dict(max_iter=0), dict(max_iter=201), dict(min_valid=0), dict(tol=-1.0), dict(tol=math.nan)):
        with pytest.raises(ValueError):
            site_diff_host(a, off, a, off, device=10 ** 6, **kw)
    with pytest.raises(ValueError):
        site_diff_host(a, off, a, np.array([0, 2, 4], np.int64), device=10 ** 6)        # one site against two
    with pytest.raises(ValueError):
        site_diff_host(a, None, a, off, device=10 ** 6)                                  # neither offsets nor a stride
    with pytest.raises(TypeError):
        site_diff_host(a, off, a, off, resp=True)                                        # K14 has the posterior


def test_refusals_of_the_read_level_layer_before_any_device_work():
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    kw = dict(device=10 ** 6, log=lambda *a: None)
    with pytest.raises(ValueError, match='diff: unknown option'):
        RL.compare_reads_llr(reads, reads, model, alt, diff=dict(resp=True), **kw)
    with pytest.raises(ValueError, match='ci_level'):
        RL.compare_reads_llr(reads, reads, model, alt, diff=dict(ci_level=1.0), **kw)
    with pytest.raises(ValueError, match='names'):
        RL.compare_reads_llr(reads, reads, model, alt, names=['chrOther'], **kw)          # the samples' chromosome is not among them
    with pytest.raises(ValueError, match='fdr method'):
        RL.compare_reads_llr(reads, reads, model, alt, fdr='holm', **kw)
    with pytest.raises(ValueError, match='min_coverage'):
        RL.compare_reads_llr(reads, reads, model, alt, min_coverage=0, **kw)
    per_position = dict(chrom=np.array(['chrT']), strand=np.array(['+']), pos=np.array([5]), base=np.array(['A']), off=np.array([0, 2]), sig=np.zeros(2))
    for pair in ((per_position, reads), (reads, per_position)):
        with pytest.raises(ValueError, match='not a read-level set'):
            RL.compare_reads_llr(pair[0], pair[1], model, alt, **kw)
    with pytest.raises(ValueError, match='same chromosome names'):                       # two pivots made with different names
        engine.match_score_rows(dict(names=['chr1']), dict(names=['chr1', 'chr2']), 1)


def test_the_command_line_refuses_before_any_device_work(tmp_path, capsys):
    from nanomod_amd import cli, container
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    r = str(tmp_path / 'reads.npz')
    container.save_reads(r, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    g = str(tmp_path / 'group.npz')
    np.savez(g, chrom=np.array(['chrT']), strand=np.array(['+']), pos=np.array([5]), base=np.array(['A']), off=np.array([0, 2]), sig=np.zeros(2))
    base = ['readdiff', '--kmerModel', r, '--altModel', r]
    assert cli.main(base + ['--wrkBase1', r, '--wrkBase2', g]) == 1 and '--wrkBase2' in capsys.readouterr().out
    assert cli.main(base + ['--wrkBase1', r, '--wrkBase2', r, '--ciLevel', '1']) == 1 and '--ciLevel' in capsys.readouterr().out
    assert cli.main(base + ['--wrkBase1', r, '--wrkBase2', str(tmp_path / 'none.npz')]) == 1 and 'does not exist' in capsys.readouterr().out
    assert cli.main(base + ['--wrkBase1', r, '--wrkBase2', r, '--minCoverage', '0']) == 1 and '--minCoverage' in capsys.readouterr().out


def test_write_site_diff_format(tmp_path):
    nan = np.nan
    sites = dict(chrom=np.array(['chrT', 'chrT']), strand=np.array(['+', '-']), pos=np.array([9, 10]), base=np.array(['A', 'C']),
                 n_reads0=np.array([30, 2], np.int32), n_reads1=np.array([31, 40], np.int32), n_valid0=np.array([30, 2], np.int32),
                 n_valid1=np.array([31, 40], np.int32), pi0=np.array([0.0, nan]), pi1=np.array([0.5, nan]), pi_pool=np.array([0.25, nan]),
                 delta=np.array([0.5, nan]), delta_lo=np.array([0.25, nan]), delta_hi=np.array([0.75, nan]), stat=np.array([12.3456, nan]),
                 p_diff=np.array([4.4e-4, nan]), diff_status=np.array([0, 1], np.uint8))
    path = str(tmp_path / 'run_site_diff.txt')
    RL.write_site_diff(path, sites)
    assert open(path).read() == ('chrT + 10 A 30 31 30 31 0.000000 0.500000 0.250000 0.500000 0.250000 0.750000 12.346 4.400E-04 0\n'
                                 'chrT - 11 C 2 40 2 40 nan nan nan nan nan nan nan nan 1\n')
    RL.write_site_diff(path, dict(sites, q=np.array([8.8e-4, nan])))
    assert open(path).read().splitlines()[0].endswith(' 4.400E-04 8.800E-04 0') and open(path).read().splitlines()[1].endswith(' nan nan 1')
