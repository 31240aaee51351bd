"""nmod_site_diff_rep (K24) without a GPU: the numpy restatement of the header's definition (tests/diff_rep_ref.py) against 50-digit
mpmath within the gates it derives, its tails against mpmath's gammainc and betainc, the package's F(1, df) quantile against
scipy and mpmath, the declaration, the export and the binding, the refusals of the Python layers before any device work, the format
of the table, the command line's two paths, and the seeded null simulation whose rates the header and profiles/site_diff_rep.txt
record.

The rates below (REF_RATES) were measured with the restatement on the seeded sites of diff_rep_ref.simulate_null, 400 per cell:
    3 v 3, rho 0:     p_cond 0.0450   p_rep 0.0400   p_rep at phi_floor 1 0.0050   p_het 0.0425
    3 v 3, rho 0.05:  p_cond 0.2025   p_rep 0.0525   p_rep at phi_floor 1 0.0250   p_het 0.3750
    3 v 3, rho 0.15:  p_cond 0.4025   p_rep 0.0575   p_rep at phi_floor 1 0.0500   p_het 0.7675
    2 v 2, rho 0.1:   p_cond 0.2775   p_rep 0.0275   p_rep at phi_floor 1 0.0025   p_het 0.5225"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import diff_rep_ref as R
import stoich_ref as SR
import readllr_ref as RF
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
PROFILE = os.path.join(ROOT, 'profiles', 'site_diff_rep.txt')

REF_RATES = {'3v3 rho 0': dict(p_cond=0.0450, p_rep=0.0400, p_rep_floor1=0.0050, p_het=0.0425),
             '3v3 rho 0.05': dict(p_cond=0.2025, p_rep=0.0525, p_rep_floor1=0.0250, p_het=0.3750),
             '3v3 rho 0.15': dict(p_cond=0.4025, p_rep=0.0575, p_rep_floor1=0.0500, p_het=0.7675),
             '2v2 rho 0.1': dict(p_cond=0.2775, p_rep=0.0275, p_rep_floor1=0.0025, p_het=0.5225)}


def _share(name, dev, gate, worst):
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0: %r' % (name, dev)
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def test_restatement_is_pinned_against_mpmath():
    """seeded sites of 3 .. 7 samples (homogeneous, overdispersed, different, shares at an end) and the constructed PHI_ZERO site: every
    output within its gate of the 50-digit solution, the tails inside their ranges"""
    rng = np.random.default_rng(2403)
    sim = lambda n, sep, p: SR.simulate_row(rng, n, sep, p)
    cases = [([sim(12, 3.0, 0.3), sim(9, 3.0, 0.3), sim(15, 3.0, 0.3)], 1, 0.0),
             ([sim(12, 1.0, 0.1), sim(9, 1.0, 0.5), sim(15, 1.0, 0.2), sim(11, 1.0, 0.7)], 2, 0.0),
             ([sim(12, 8.0, 0.1), sim(9, 8.0, 0.15), sim(15, 8.0, 0.8), sim(11, 8.0, 0.9), sim(20, 8.0, 0.85)], 2, 1.0),
             ([sim(8, 3.0, 0.0), sim(9, 3.0, 0.4), sim(7, 3.0, 1.0), sim(11, 3.0, 0.6), sim(6, 3.0, 0.5), sim(10, 3.0, 0.5), sim(5, 3.0, 0.2)], 3, 0.0),
             ([sim(30, 0.3, 0.5), sim(30, 0.3, 0.5), sim(30, 0.3, 0.5), sim(30, 0.3, 0.5)], 3, 0.5),
             ([np.full(6, -40.0), np.full(5, -40.0), np.full(7, 40.0), np.full(4, 40.0)], 2, 0.0),
             ([np.full(6, -40.0), np.full(5, -40.0), np.full(7, 40.0), np.full(4, 40.0)], 2, 1.0)]
    worst = {}
    for rows, nc, floor in cases:
        r, x = R.site(rows, nc, phi_floor=floor, interval=False), R.exact_site(rows, nc, phi_floor=floor)
        assert r['gates'] is not None and r['status'] & ~(R.POOL_AT_END | R.PHI_ZERO) == 0, r['status']
        g = r['gates']
        for k in range(len(rows)):
            _share('pi_s', abs(float(x['pi_s'][k] - r['pi_s'][k])), g['pi_s'][k], worst)
        for f in ('pi0', 'pi1', 'pi_pool', 'delta', 'stat_cond', 'stat_het', 'phi'):
            _share(f, abs(float(x[f] - r[f])), g[f], worst)
        for f in ('p_cond', 'p_het', 'p_rep'):
            lo, hi = g[f]
            assert lo <= float(x[f]) <= hi, (f, lo, float(x[f]), hi)
    assert R.site(cases[5][0], 2)['status'] & R.PHI_ZERO and R.site(cases[5][0], 2)['p_rep'] == R.DBL_MIN
    plainF = R.site(cases[6][0], 2, phi_floor=1.0)
    assert plainF['status'] & R.PHI_ZERO == 0 and plainF['phi'] == 0.0 and plainF['p_rep'] == R.t_two_sided(plainF['stat_cond'], 2)
    print('worst deviation as a share of its gate: %s' % ', '.join('%s %.3g' % kv for kv in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_the_tails_against_mpmath():
    """chi2_df by the header's two closed forms against gammainc at odd and even df, the F(1, df) tail against betainc at df 1 .. 14"""
    import mpmath as mp
    worst = dict(chi2=0.0, F=0.0)
    with mp.workdps(50):
        for df in range(1, 15):
            for stat in (1e-9, 0.01, 0.5, 1.0, 3.84, 10.0, 40.0, 200.0, 1200.0):
                want = mp.gammainc(mp.mpf(df) / 2, mp.mpf(stat) / 2, mp.inf, regularized=True)
                worst['chi2'] = max(worst['chi2'], abs(float((R.chi2_sf(stat, df) - want) / want)))
                want = mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, mp.mpf(df) / (df + mp.mpf(stat)), regularized=True)
                worst['F'] = max(worst['F'], abs(float((R.t_two_sided(stat, df) - want) / want)))
    print('worst relative error: chi2 tail %.3g, F(1, df) tail %.3g' % (worst['chi2'], worst['F']))
    assert worst['chi2'] <= R.P_TAIL and worst['F'] <= R.P_TAIL, worst
    assert R.chi2_sf(0.0, 3) == 1.0 and R.t_two_sided(0.0, 3) == 1.0 and R.t_two_sided(math.inf, 3) == 0.0


def test_the_quantile_helper_against_scipy():
    """engine._f1_quantile, the package's own inverse of the t tail: scipy.stats.t.ppf squared at df 1 .. 14 (scipy's own error against
    mpmath reaches 5e-11 there: the bound is 1e-9) and mpmath's root of the tail at 1e-12"""
    import mpmath as mp
    from scipy import stats
    for df in range(1, 15):
        for level in (0.5, 0.8, 0.9, 0.95, 0.99, 0.999):
            got, want = engine._f1_quantile(level, df), float(stats.t.ppf(0.5 * (1.0 + level), df)) ** 2
            assert abs(got - want) <= 1e-9 * want, (df, level, got, want)
            with mp.workdps(40):
                f = lambda q: mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, df / (df + q), regularized=True) - (1 - mp.mpf(level))
                exact = mp.findroot(f, mp.mpf(want))
                assert abs(got - exact) <= 1e-12 * exact, (df, level, got, float(exact))
    o, G, nc = engine._rep_opts(5, 2, 3, 0.95, 0.0, 60, 1e-12)
    assert (G, nc) == (5, 2) and abs(o.ci_drop - R.f1_quantile(0.95, 3)) <= 1e-9 * o.ci_drop and o.phi_floor == 0.0


def test_header_symbol_and_abi():
    text = open(HEADER).read()
    assert re.search(r'#define NMOD_REP_MAX_SAMPLES (\d+)', text).group(1) == str(R.MAX_SAMPLES) == str(L.REP_MAX_SAMPLES)
    assert ('NMOD_REP_TOO_FEW = 1, NMOD_REP_FLAT = 2, NMOD_REP_NOT_CONVERGED = 4, NMOD_REP_POOL_AT_END = 8, NMOD_REP_PHI_ZERO = 16,\n'
            '       NMOD_REP_TOO_LARGE = 32') in text
    assert (L.REP_TOO_FEW, L.REP_FLAT, L.REP_NOT_CONVERGED, L.REP_POOL_AT_END, L.REP_PHI_ZERO, L.REP_TOO_LARGE) == (1, 2, 4, 8, 16, 32) == \
        (R.TOO_FEW, R.FLAT, R.NOT_CONVERGED, R.POOL_AT_END, R.PHI_ZERO, R.TOO_LARGE)
    for phrase in ('int nmod_site_diff_rep(const nmod_params* prm', 'two conditions, no covariates', 'every sample must cover the site',
                   'one dispersion per site', 'little\n * power', 'both k-mer tables are taken as right', 'G = 2 is refused'):
        assert phrase in text, phrase
    assert re.search(r'#define NMOD_ABI_VERSION\s+4\b', text) and L.NMOD_ABI_VERSION == 4
    assert C.sizeof(L.NmodRepOpts) == 40 and C.sizeof(L.NmodRepOut) == 8 + 16 * 8
    assert L.REP_FIELDS == R.FIELDS
    lib = L.load()
    assert lib.nmod_abi_version() == 4 and lib.nmod_site_diff_rep.argtypes is not None
    syms = subprocess.run(['nm', '-D', '--defined-only', os.path.join(ROOT, 'nanomod_amd', 'libnanomod_hip.so')], capture_output=True, text=True, check=True)
    assert re.search(r' T nmod_site_diff_rep$', syms.stdout, re.M) and re.search(r' T nmod_site_diff$', syms.stdout, re.M)


def test_the_header_and_the_profile_record_the_measured_rates():
    text, prof = open(HEADER).read(), open(PROFILE).read()
    for name, rates in REF_RATES.items():
        line = 'p_cond %.3f   p_rep %.3f   p_rep at phi_floor 1 %.3f   p_het %.3f' % tuple(
            float('%.3f' % (rates[k] + 1e-9)) for k in ('p_cond', 'p_rep', 'p_rep_floor1', 'p_het'))
        assert line in text, (name, line)
        assert 'p_cond %.4f  p_rep %.4f  p_rep(phi_floor 1) %.4f  p_het %.4f' % tuple(rates[k] for k in ('p_cond', 'p_rep', 'p_rep_floor1', 'p_het')) in prof, name


def test_refusals_before_any_device_work():
    a = np.array([1.0, -1.0, 2.0, 0.5, 1.0, -1.0, 2.0, 0.5, 3.0])
    off = np.array([0, 3, 6, 9], np.int64)
    ok = dict(device=10 ** 6)
    for kw in (dict(ci_level=1.0), dict(ci_level=0.0), dict(max_iter=0), dict(max_iter=201), dict(min_valid=0), dict(tol=-1.0), dict(tol=math.nan),
               dict(phi_floor=-0.5), dict(phi_floor=math.inf), dict(phi_floor=math.nan)):
        with pytest.raises(ValueError):
            engine.site_diff_rep_host(a, off, 3, 1, **ok, **kw)
    for G, nc in ((2, 1), (17, 3), (3, 0), (3, 3), (3.5, 1), (4, 1.5)):
        with pytest.raises(ValueError):
            engine.site_diff_rep_host(a, off, G, nc, **ok)
    with pytest.raises(ValueError, match='n_samples rows per site'):
        engine.site_diff_rep_host(a, np.array([0, 2, 4, 6, 9], np.int64), 3, 1, **ok)    # four rows of three samples
    with pytest.raises(ValueError):
        engine.site_diff_rep_host(a, None, 3, 1, **ok)                                    # CSR only
    with pytest.raises(ValueError):
        engine.match_score_rows_multi([dict(names=['chr1'])] * 2, 1, 1)                   # two samples: match_score_rows
    with pytest.raises(ValueError, match='same chromosome names'):
        engine.match_score_rows_multi([dict(names=['chr1']), dict(names=['chr1']), dict(names=['chr1', 'chr2'])], 1, 1)


def test_refusals_of_the_read_level_layer_before_any_device_work():
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    kw = dict(device=10 ** 6, log=lambda *a: None)
    with pytest.raises(ValueError, match='diff: unknown option'):
        RL.compare_reads_llr_rep([reads, reads], [reads], model, alt, diff=dict(resp=True), **kw)
    with pytest.raises(ValueError, match='phi_floor'):
        RL.compare_reads_llr_rep([reads, reads], [reads], model, alt, diff=dict(phi_floor=-1.0), **kw)
    with pytest.raises(ValueError, match='n_samples'):
        RL.compare_reads_llr_rep([reads], [reads], model, alt, **kw)                       # two samples: compare_reads_llr
    with pytest.raises(ValueError, match='n_control'):
        RL.compare_reads_llr_rep([], [reads, reads, reads], model, alt, **kw)
    with pytest.raises(ValueError, match='names'):
        RL.compare_reads_llr_rep([reads, reads], [reads], model, alt, names=['chrOther'], **kw)
    with pytest.raises(ValueError, match='fdr method'):
        RL.compare_reads_llr_rep([reads, reads], [reads], model, alt, fdr='holm', **kw)


def test_write_site_diff_rep_format(tmp_path):
    nan = np.nan
    sites = dict(chrom=np.array(['chrT', 'chrT']), strand=np.array(['+', '-']), pos=np.array([9, 10]), base=np.array(['A', 'C']), n_samples=3,
                 n_control=1, n_valid=np.array([[30, 31, 29], [2, 40, 41]], np.int32), pi_s=np.array([[0.0, 0.5, 0.625], [nan, nan, nan]]),
                 pi0=np.array([0.0, nan]), pi1=np.array([0.5, nan]), pi_pool=np.array([0.25, nan]), delta=np.array([0.5, nan]),
                 delta_lo=np.array([0.25, nan]), delta_hi=np.array([0.75, nan]), stat_cond=np.array([12.3456, nan]), p_cond=np.array([4.4e-4, nan]),
                 stat_het=np.array([1.5, nan]), p_het=np.array([0.2207, nan]), phi=np.array([1.5, nan]), p_rep=np.array([0.0543, nan]),
                 rep_status=np.array([0, 1], np.uint8))
    path = str(tmp_path / 'run_site_diff_rep.txt')
    RL.write_site_diff_rep(path, sites)
    assert open(path).read() == ('chrT + 10 A 3 30 0.000000 31 0.500000 29 0.625000 0.000000 0.500000 0.250000 0.500000 0.250000 0.750000 12.346 '
                                 '4.400E-04 1.500 2.207E-01 1.500 5.430E-02 0\n'
                                 'chrT - 11 C 3 2 nan 40 nan 41 nan nan nan nan nan nan nan nan nan nan nan nan nan 1\n')
    RL.write_site_diff_rep(path, dict(sites, q=np.array([8.8e-2, nan])))
    lines = open(path).read().splitlines()
    assert lines[0].endswith(' 5.430E-02 8.800E-02 0') and lines[1].endswith(' nan nan 1') and len(lines[0].split()) == 5 + 2 * 3 + 12 + 2


def test_readdiff_with_single_files_takes_the_two_sample_path(tmp_path, monkeypatch, capsys):
    """one container each: compare_reads_llr and <FileID>_site_diff.txt as before; three in all: compare_reads_llr_rep and
    <FileID>_site_diff_rep.txt with --phiFloor handed on (the chains themselves are replaced: no device here)"""
    from nanomod_amd import cli, container, kmermodel
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    r = str(tmp_path / 'reads.npz')
    container.save_reads(r, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    seen = []
    monkeypatch.setattr(kmermodel, 'load_kmer_model', lambda p: dict(path=p))
    monkeypatch.setattr(RL, 'compare_reads_llr', lambda r0, r1, m, a, **kw: seen.append(('two', kw)) or 'S2')
    monkeypatch.setattr(RL, 'compare_reads_llr_rep', lambda l0, l1, m, a, **kw: seen.append(('rep', len(l0), len(l1), kw)) or 'SR')
    monkeypatch.setattr(RL, 'write_site_diff', lambda path, sites: seen.append(('w2', os.path.basename(path), sites)))
    monkeypatch.setattr(RL, 'write_site_diff_rep', lambda path, sites: seen.append(('wr', os.path.basename(path), sites)))
    base = ['readdiff', '--kmerModel', r, '--altModel', r, '--FileID', 'run', '--outFolder', str(tmp_path / 'out')]
    assert cli.main(base + ['--wrkBase1', r, '--wrkBase2', r]) == 0
    assert [s[0] for s in seen] == ['two', 'w2'] and seen[1][1:] == ('run_site_diff.txt', 'S2') and 'phi_floor' not in seen[0][1]['diff']
    del seen[:]
    assert cli.main(base + ['--wrkBase1', r + ',' + r, '--wrkBase2', r, '--phiFloor', '1', '--fdr', 'bh']) == 0
    assert [s[0] for s in seen] == ['rep', 'wr'] and seen[0][1:3] == (2, 1) and seen[1][1:] == ('run_site_diff_rep.txt', 'SR')
    assert seen[0][3]['diff'] == dict(min_valid=3, ci_level=0.95, phi_floor=1.0) and seen[0][3]['fdr'] == 'bh'
    capsys.readouterr()
    assert cli.main(base + ['--wrkBase1', r + ',' + r, '--wrkBase2', r, '--phiFloor', '-1']) == 1 and '--phiFloor' in capsys.readouterr().out
    assert cli.main(base + ['--wrkBase1', r + ',' + str(tmp_path / 'none.npz'), '--wrkBase2', r]) == 1 and 'does not exist' in capsys.readouterr().out
    assert cli.main(base + ['--wrkBase1', ','.join([r] * 16), '--wrkBase2', r]) == 1 and 'at most 16' in capsys.readouterr().out


@pytest.mark.parametrize('cell', range(len(R.SIM_CELLS)))
def test_null_rates_of_the_seeded_simulation(cell):
    """400 seeded null sites per cell under the restatement: the 5 % rejection rates are the recorded ones (REF_RATES; p_rep within
    three binomial standard errors at 400 sites), and where the replicates are overdispersed p_rep rejects less often than p_cond"""
    name, k0, k1, rho = R.SIM_CELLS[cell]
    rates, n = R.simulate_null(cell)
    print('%s: %d sites with an estimate; rejected at 5 %%: %s' % (name, n, ', '.join('%s %.4f' % kv for kv in rates.items())))
    assert n >= 0.95 * R.SIM_SITES
    ref = REF_RATES[name]
    se = math.sqrt(ref['p_rep'] * (1.0 - ref['p_rep']) / R.SIM_SITES)
    assert abs(rates['p_rep'] - ref['p_rep']) <= 3.0 * se, (rates['p_rep'], ref['p_rep'], se)
    if rho > 0.0:
        assert rates['p_rep'] < rates['p_cond'], rates
