"""nmod_rep_prior and nmod_site_diff_rep_mod (K25) without a GPU: the numpy restatement (tests/diff_mod_ref.py) and the device's own
scalar functions (special_math.hpp, compiled for the host) against 50-digit mpmath at the deviations measured over the grids below;
the declaration, the export and the binding; the refusals of the Python layers before any device work; the format of the two
files; the command line's option; and the seeded null and planted simulations whose rates the header and
profiles/site_diff_mod.txt record.

The tolerances are not chosen: diff_mod_ref.MEASURED and DEVICE_MEASURED hold the worst relative deviations these tests measured,
and every test holds its function to MARGIN (2) times its figure and prints what it measures now.

The rates (REF_RATES): rejected at the 5 % level of 400 seeded sites per cell, the prior fitted on the cell; `planted`: the other
condition's replicates drawn around 0.3 + the planted difference.
    3 v 3, rho 0:     null     p_cond 0.0450  p_rep 0.0400  moderated 0.0450   d0 inf
                      planted  p_cond 0.3675  p_rep 0.2500  moderated 0.3625   d0 inf      (+0.12)
    3 v 3, rho 0.05:  null     p_cond 0.2025  p_rep 0.0525  moderated 0.0475   d0 192.9
                      planted  p_cond 0.6950  p_rep 0.3100  moderated 0.4250   d0 46.7     (+0.22)
    3 v 3, rho 0.15:  null     p_cond 0.4025  p_rep 0.0575  moderated 0.0525   d0 inf
                      planted  p_cond 0.9025  p_rep 0.3275  moderated 0.5250   d0 inf      (+0.36)
    2 v 2, rho 0.1:   null     p_cond 0.2775  p_rep 0.0275  moderated 0.0325   d0 inf
                      planted  p_cond 0.9850  p_rep 0.4000  moderated 0.8750   d0 inf      (+0.50)"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import diff_mod_ref as M
import diff_rep_ref as R
import readllr_ref as RF
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL
from nanomod_amd.engine import rep_prior_host              # K25's entry: without it nothing here can pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
PROFILE = os.path.join(ROOT, 'profiles', 'site_diff_mod.txt')
CSRC = os.path.join(ROOT, 'nanomod_amd', 'csrc')

REF_RATES = {('3v3 rho 0', False): (0.0450, 0.0400, 0.0450), ('3v3 rho 0', True): (0.3675, 0.2500, 0.3625),
             ('3v3 rho 0.05', False): (0.2025, 0.0525, 0.0475), ('3v3 rho 0.05', True): (0.6950, 0.3100, 0.4250),
             ('3v3 rho 0.15', False): (0.4025, 0.0575, 0.0525), ('3v3 rho 0.15', True): (0.9025, 0.3275, 0.5250),
             ('2v2 rho 0.1', False): (0.2775, 0.0275, 0.0325), ('2v2 rho 0.1', True): (0.9850, 0.4000, 0.8750)}


def _mp():
    import mpmath as mp
    return mp


def _rel(got, exact):
    mp = _mp()
    with mp.workdps(50):
        return float(abs(mp.mpf(float(got)) - exact) / abs(exact))


def _hold(name, worst, table=M.MEASURED):
    print('%s: worst relative deviation from mpmath %.3g (recorded %.3g, held to %g times that)' % (name, worst, table[name], M.MARGIN))
    assert worst <= M.MARGIN * table[name], (name, worst)


# ------------------------------------------------------------------------------------------------- the restatement against mpmath
def test_the_inverse_trigamma_against_mpmath():
    rng = np.random.default_rng(2550)
    xs = np.exp(rng.uniform(math.log(1e-6), math.log(1e7), 400))
    _hold('trigamma_inverse', max(_rel(M.trigamma_inverse(float(x)), M.exact_trigamma_inverse(float(x))) for x in xs))
    assert M.trigamma_inverse(2e7) == 1.0 / math.sqrt(2e7) and M.trigamma_inverse(1e-7) == 1e7 and math.isnan(M.trigamma_inverse(math.nan))


def test_the_fit_against_mpmath():
    """600 sites of 1.9 F(df, d0) per cell of df 1, 2, 4, 14 x d0 0.7, 3, 12, 80; the e_i are taken as exact, so that what is measured
    is the two-pass variance, psi'^-1 and the exponent (the worst d0 is a large one: evar is then a small difference)"""
    rng = np.random.default_rng(2551)
    wd = ws = 0.0
    finite = 0
    for df in (1, 2, 4, 14):
        for d0t in (0.7, 3.0, 12.0, 80.0):
            phi = 1.9 * (rng.chisquare(df, 600) / df) / (rng.chisquare(d0t, 600) / d0t)
            p = M.rep_prior(phi, np.zeros(600, np.uint8), df)
            d0, s0 = M.exact_solve(p['e'], df)
            assert math.isinf(p['d0']) == (d0 == _mp().inf)
            ws = max(ws, _rel(p['s0sq'], s0))
            if not math.isinf(p['d0']):
                finite += 1
                wd = max(wd, _rel(p['d0'], d0))
                assert p['df_tot'] == df + p['d0'] and p['n_used'] == 600.0 and p['n_zero'] == 0.0
    assert finite >= 12
    _hold('d0', wd)
    _hold('s0sq', ws)


def test_the_quantile_and_the_tail_against_mpmath():
    wq = max(_rel(M.f1_quantile(level, nu), M.exact_f1_quantile(level, nu)) for nu in M.NUS for level in M.LEVELS)
    _hold('f1_quantile', wq)
    wt = max(_rel(M.tail(F, nu), M.exact_tail(F, nu)) for nu in M.NUS for F in (1e-3, 0.1, 1.0, 3.84, 10.0, 50.0, 400.0))
    _hold('tail', wt)
    assert M.tail(0.0, 3.7) == 1.0 and M.tail(math.inf, 3.7) == 0.0
    # the package's own helper (integer df) and diff_rep_ref's agree with it where they apply
    for df in (1, 2, 4, 14):
        assert abs(engine._f1_quantile(0.95, df) - M.f1_quantile(0.95, df)) <= 1e-12 * M.f1_quantile(0.95, df)
        assert abs(R.t_two_sided(3.84, df) - M.tail(3.84, df)) <= 1e-11 * M.tail(3.84, df)


def test_the_three_cases_of_the_record():
    phi = np.array([0.5, 3.0, 1.2, 0.0, np.nan, np.inf, 7.0, 2.0, -0.0])
    status = np.array([0, 0, R.NOT_CONVERGED, 0, 0, 0, R.TOO_FEW, R.POOL_AT_END, R.PHI_ZERO], np.uint8)
    p = M.rep_prior(phi, status, 2)
    assert (p['n_used'], p['n_zero']) == (4.0, 2.0) and len(p['e']) == 4
    assert abs(p['emean'] - (np.log([0.5, 3.0, 1.2, 2.0]).mean() - M.digamma(1.0))) < 1e-15
    one = M.rep_prior(phi[:1], status[:1], 2)
    assert one['d0'] == 0.0 and math.isnan(one['s0sq']) and one['df_tot'] == 2.0 and one['ci_drop'] == M.f1_quantile(0.95, 2) and math.isnan(one['evar'])
    none = M.rep_prior(phi[:0], status[:0], 3)
    assert none['d0'] == 0.0 and math.isnan(none['emean']) and none['n_used'] == 0.0
    same = M.rep_prior(np.full(50, 1.7), np.zeros(50, np.uint8), 4)
    assert same['evar'] < 0.0 and same['d0'] == math.inf and abs(same['s0sq'] - math.exp(same['emean'])) < 1e-15
    assert same['ci_drop'] == M.f1_quantile(0.95, math.inf) and abs(same['ci_drop'] - 3.841458820694124) < 1e-12
    # the moderated dispersion
    rec = np.array([3.7, 1.3, 5.7, 1.0, 0, 0, 0, 0])
    assert M.phi_post_of(2.0, rec, 2) == (3.7 * 1.3 + 2 * 2.0) / (3.7 + 2) and M.phi_post_of(2.0, M.record(one), 2) == 2.0
    assert M.phi_post_of(2.0, M.record(same), 4) == same['s0sq']
    assert not M.prior_bad(M.record(one)) and M.prior_bad([math.nan, 1, 2, 3]) and M.prior_bad([1.0, math.nan, 3, 3]) and M.prior_bad([1, 1, -1, 3])


# --------------------------------------------------------------------------------------------- the device's functions on the host
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
// polymath <function> <in> <out>: pairs of doubles in (the second unused by the one-argument functions), one double out each, raw
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[2], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END); long n = ftell(f) / 16; fseek(f, 0, SEEK_SET);
  double* x = (double*)malloc(16 * (n > 0 ? n : 1));
  if (fread(x, 16, n, f) != (size_t)n) return 4;
  fclose(f);
  for (long i = 0; i < n; ++i) {
    const double a = x[2 * i], b = x[2 * i + 1];
    if (!strcmp(argv[1], "digamma")) x[i] = nmod::digamma(a);
    else if (!strcmp(argv[1], "trigamma")) x[i] = nmod::trigamma(a);
    else if (!strcmp(argv[1], "tetragamma")) x[i] = nmod::tetragamma(a);
    else if (!strcmp(argv[1], "trigamma_inverse")) x[i] = nmod::trigamma_inverse(a);
    else if (!strcmp(argv[1], "f1_quantile")) x[i] = nmod::f1_quantile(a, b);
    else return 5;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(x, 8, n, f) != (size_t)n) return 6;
  fclose(f);
  return 0;
}
'''


@pytest.fixture(scope='module')
def polymath(tmp_path_factory):
    """special_math.hpp through a stub <hip/hip_runtime.h> that defines the HIP qualifiers away (tests/test_tail_math_host.py's method):
    the arithmetic of the functions with glibc's exp and log where the device has ocml's"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('polymath')
    os.makedirs(d / 'stub' / 'hip')
    (d / 'stub' / 'hip' / 'hip_runtime.h').write_text(STUB)
    (d / 'main.cpp').write_text(MAIN)
    exe = str(d / 'polymath')
    subprocess.check_call([cxx, '-O2', '-std=c++17', '-ffp-contract=off', '-I', str(d / 'stub'), '-I', CSRC, str(d / 'main.cpp'), '-o', exe, '-lm'])

    def run(fn, a, b=None):
        a = np.asarray(a, dtype=np.float64)
        x = np.stack([a, np.zeros_like(a) if b is None else np.asarray(b, dtype=np.float64)], axis=1)
        np.ascontiguousarray(x).tofile(str(d / 'in.bin'))
        subprocess.check_call([exe, fn, str(d / 'in.bin'), str(d / 'out.bin')])
        out = np.fromfile(str(d / 'out.bin'), dtype=np.float64)
        assert out.shape == a.shape
        return out
    return run


def test_the_device_polygammas_against_mpmath(polymath):
    mp = _mp()
    rng = np.random.default_rng(2552)
    xs = np.concatenate([np.exp(rng.uniform(math.log(1e-3), math.log(1e8), 4000)), np.arange(1, 15) / 2.0])
    with mp.workdps(50):
        for name, k in (('digamma', 0), ('trigamma', 1), ('tetragamma', 2)):
            got = polymath(name, xs)
            ref = [mp.polygamma(k, mp.mpf(float(x))) for x in xs]
            # digamma crosses 0 at 1.4616: its deviation is taken relative to max(1, |psi|)
            worst = max(float(abs(mp.mpf(float(g)) - r) / (max(1, abs(r)) if k == 0 else abs(r))) for g, r in zip(got, ref))
            _hold(name, worst, M.DEVICE_MEASURED)
    ys = np.exp(rng.uniform(math.log(1e-6), math.log(1e7), 500))
    got = polymath('trigamma_inverse', ys)
    _hold('trigamma_inverse', max(_rel(g, M.exact_trigamma_inverse(float(y))) for g, y in zip(got, ys)), M.DEVICE_MEASURED)
    assert polymath('trigamma_inverse', [2e7])[0] == 1.0 / math.sqrt(2e7) and polymath('trigamma_inverse', [1e-7])[0] == 1e7


def test_the_device_quantile_against_mpmath(polymath):
    """over nu integer, fractional, 1e6 and inf and the levels 0.9, 0.95, 0.999.  The worst, 1.9e-11, is nu = 1 at 0.999 (t = 637),
    where student_t_two_sided's log1p(-y) has y within 2.5e-6 of 1; without that point the worst is 2.6e-13"""
    pairs = [(level, nu) for nu in M.NUS for level in M.LEVELS]
    got = polymath('f1_quantile', [p[0] for p in pairs], [p[1] for p in pairs])
    dev = [_rel(g, M.exact_f1_quantile(level, nu)) for g, (level, nu) in zip(got, pairs)]
    _hold('f1_quantile', max(dev), M.DEVICE_MEASURED)
    rest = max(d for d, (level, nu) in zip(dev, pairs) if (level, nu) != (0.999, 1))
    print('without nu = 1 at 0.999: %.3g' % rest)
    assert rest <= 1e-12


# ------------------------------------------------------------------------------------------- the declaration, export and binding
def test_header_symbols_and_abi():
    text = open(HEADER).read()
    assert re.search(r'#define NMOD_REP_PRIOR_WORDS (\d+)', text).group(1) == str(L.REP_PRIOR_WORDS) == str(M.PRIOR_WORDS) == '8'
    assert re.search(r'#define NMOD_REP_PRIOR_CHUNK (\d+)', text).group(1) == str(L.REP_PRIOR_CHUNK) == str(M.PRIOR_CHUNK)
    assert 'enum { NMOD_REP_BAD_PRIOR = 64 };' in text and L.REP_BAD_PRIOR == M.BAD_PRIOR == 64
    assert L.REP_PRIOR_FIELDS == M.PRIOR_FIELDS and len(L.REP_PRIOR_FIELDS) == L.REP_PRIOR_WORDS
    for phrase in ('int nmod_rep_prior(const nmod_params* prm', 'int nmod_site_diff_rep_mod(const nmod_params* prm', "limma's fitFDist",
                   'no trend in coverage or share', 'zeros are left out of the fit', 'no robust (winsorised) fit', 'is an approximation',
                   'opts->ci_drop is checked as before and then IGNORED', 'The three fits run twice', 'first step of relative size below 1e-8'):
        assert phrase in text, phrase
    assert re.search(r'#define NMOD_ABI_VERSION\s+4\b', text) and L.NMOD_ABI_VERSION == 4
    assert C.sizeof(L.NmodRepOpts) == 40 and C.sizeof(L.NmodRepOut) == 8 + 16 * 8                     # K24's structs keep their sizes
    lib = L.load()
    assert lib.nmod_abi_version() == 4 and len(lib.nmod_rep_prior.argtypes) == 7 and len(lib.nmod_site_diff_rep_mod.argtypes) == 10
    syms = subprocess.run(['nm', '-D', '--defined-only', os.path.join(ROOT, 'nanomod_amd', 'libnanomod_hip.so')], capture_output=True, text=True, check=True)
    assert re.search(r' T nmod_rep_prior$', syms.stdout, re.M) and re.search(r' T nmod_site_diff_rep_mod$', syms.stdout, re.M)
    assert re.search(r' T nmod_site_diff_rep$', syms.stdout, re.M)
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert ' rep_prior.o ' in mk and '$(OBJDIR)/rep_prior.o: CXXFLAGS += -ffp-contract=off' in mk


def test_refusals_before_any_device_work():
    ok = dict(device=10 ** 6)
    phi, status = np.array([1.0, 2.0]), np.zeros(2, np.uint8)
    for kw in (dict(df=0), dict(df=15), dict(df=1.5), dict(ci_level=0.0), dict(ci_level=1.0), dict(ci_level=math.nan)):
        with pytest.raises(ValueError):
            rep_prior_host(phi, status, **dict(dict(df=2), **kw), **ok)
    with pytest.raises(ValueError, match='one length'):
        engine.rep_prior_host(phi, np.zeros(3, np.uint8), 2, **ok)
    a, off = np.array([1.0, -1.0, 2.0, 0.5, 1.0, -1.0, 2.0, 0.5, 3.0]), np.array([0, 3, 6, 9], np.int64)
    for prior in (np.zeros(7), np.zeros((2, 4)), dict(d0=1.0)):
        with pytest.raises((ValueError, KeyError)):
            engine.site_diff_rep_host(a, off, 3, 1, prior=prior, **ok)
    rec = engine.rep_prior_record(dict(zip(L.REP_PRIOR_FIELDS, range(8))))
    assert rec.dtype == np.float64 and rec.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert engine._rep_shapes(5, 3, True, moderated=True)['phi_post'] == ('float64', 5) and 'phi_post' not in engine._rep_shapes(5, 3, True)
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    with pytest.raises(ValueError, match='n_samples'):
        RL.compare_reads_llr_rep([reads], [reads], model, alt, moderate=True, device=10 ** 6, log=lambda *a: None)


def _sites():
    nan = np.nan
    return dict(chrom=np.array(['chrT', 'chrT']), strand=np.array(['+', '-']), pos=np.array([9, 10]), base=np.array(['A', 'C']), n_samples=3,
                n_control=1, n_valid=np.array([[30, 31, 29], [2, 40, 41]], np.int32), pi_s=np.array([[0.0, 0.5, 0.625], [nan, nan, nan]]),
                pi0=np.array([0.0, nan]), pi1=np.array([0.5, nan]), pi_pool=np.array([0.25, nan]), delta=np.array([0.5, nan]),
                delta_lo=np.array([0.25, nan]), delta_hi=np.array([0.75, nan]), stat_cond=np.array([12.3456, nan]), p_cond=np.array([4.4e-4, nan]),
                stat_het=np.array([1.5, nan]), p_het=np.array([0.2207, nan]), phi=np.array([1.5, nan]), p_rep=np.array([0.0143, nan]),
                phi_post=np.array([1.2345, nan]), df_tot=4.7, rep_status=np.array([0, 1], np.uint8),
                rep_prior=dict(d0=3.7, s0sq=1.25, df_tot=4.7, ci_drop=6.5, n_used=1.0, n_zero=0.0, emean=0.1, evar=0.5))


def test_write_site_diff_mod_format(tmp_path):
    path = str(tmp_path / 'run_site_diff_mod.txt')
    RL.write_site_diff_mod(path, _sites())
    assert open(path).read() == ('chrT + 10 A 3 30 0.000000 31 0.500000 29 0.625000 0.000000 0.500000 0.250000 0.500000 0.250000 0.750000 12.346 '
                                 '4.400E-04 1.500 2.207E-01 1.500 1.430E-02 1.234 4.7 0\n'
                                 'chrT - 11 C 3 2 nan 40 nan 41 nan nan nan nan nan nan nan nan nan nan nan nan nan nan 4.7 1\n')
    assert open(str(tmp_path / 'run_rep_prior.txt')).read() == 'd0 3.7000000000000002\ns0sq 1.25\ndf_tot 4.7000000000000002\nci_drop 6.5\nn_used 1\nn_zero 0\nemean 0.10000000000000001\nevar 0.5\n'
    RL.write_site_diff_mod(path, dict(_sites(), q=np.array([8.8e-2, np.nan])), prior_path=str(tmp_path / 'elsewhere.txt'))
    lines = open(path).read().splitlines()
    assert lines[0].endswith(' 1.430E-02 1.234 4.7 8.800E-02 0') and lines[1].endswith(' nan nan 4.7 nan 1') and len(lines[0].split()) == 5 + 2 * 3 + 12 + 2 + 2
    assert open(str(tmp_path / 'elsewhere.txt')).read().startswith('d0 3.7')


def test_readdiff_moderate_option(tmp_path, monkeypatch, capsys):
    """--moderate 1 hands moderate=True on and writes through write_site_diff_mod; without it the call and the file are K24's, with
    no new keyword; with one container each it is refused (the chains themselves are replaced: no device here)"""
    from nanomod_amd import cli, container, kmermodel
    reads, model, alt, _ = RF.chain_inputs(n_reads=4, shift_sd=2.0)
    r = str(tmp_path / 'reads.npz')
    container.save_reads(r, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    seen = []
    monkeypatch.setattr(kmermodel, 'load_kmer_model', lambda p: dict(path=p))
    monkeypatch.setattr(RL, 'compare_reads_llr_rep', lambda l0, l1, m, a, **kw: seen.append(('rep', len(l0), len(l1), kw)) or 'SR')
    monkeypatch.setattr(RL, 'write_site_diff_rep', lambda path, sites: seen.append(('wr', os.path.basename(path), sites)))
    monkeypatch.setattr(RL, 'write_site_diff_mod', lambda path, sites: seen.append(('wm', os.path.basename(path), sites)))
    base = ['readdiff', '--kmerModel', r, '--altModel', r, '--FileID', 'run', '--outFolder', str(tmp_path / 'out'), '--wrkBase1', r + ',' + r]
    assert cli.main(base + ['--wrkBase2', r + ',' + r, '--moderate', '1', '--fdr', 'by']) == 0
    assert [s[0] for s in seen] == ['rep', 'wm'] and seen[1][1:] == ('run_site_diff_mod.txt', 'SR')
    assert seen[0][3]['moderate'] is True and seen[0][3]['fdr'] == 'by' and seen[0][3]['diff'] == dict(min_valid=3, ci_level=0.95, phi_floor=0.0)
    assert 'run_site_diff_mod.txt' in capsys.readouterr().out
    del seen[:]
    assert cli.main(base + ['--wrkBase2', r]) == 0
    assert [s[0] for s in seen] == ['rep', 'wr'] and 'moderate' not in seen[0][3] and seen[1][1] == 'run_site_diff_rep.txt'
    capsys.readouterr()
    assert cli.main(['readdiff', '--kmerModel', r, '--altModel', r, '--wrkBase1', r, '--wrkBase2', r, '--moderate', '1']) == 1
    assert '--moderate' in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------- calibration and power
@pytest.mark.parametrize('cell', range(len(R.SIM_CELLS)))
def test_rates_of_the_seeded_simulations(cell):
    """400 seeded sites per cell, null (diff_rep_ref's own sites) and planted, the prior fitted on the cell.  Only relations are
    asserted: on the planted cell the moderated test rejects at least as many sites as K24's p_rep, on a null cell with rho > 0
    fewer than p_cond; the rates themselves are the recorded ones (REF_RATES: the simulation is seeded), and K24's p_rep rejects
    between a fifth and four fifths of the planted sites, which is how the planted differences were chosen"""
    name, k0, k1, rho = R.SIM_CELLS[cell]
    null, planted = M.rates(cell, False), M.rates(cell, True)
    for what, r in (('null', null), ('planted +%g' % M.PLANTED[cell], planted)):
        print('%s, %s: %d sites; rejected at 5 %%: p_cond %.4f, p_rep %.4f, moderated %.4f; d0 %g, s0^2 %.4g, %d zero(s)'
              % (name, what, r['n'], r['p_cond'], r['p_rep'], r['p_mod'], r['d0'], r['s0sq'], r['n_zero']))
    assert null['n'] >= 0.95 * R.SIM_SITES and planted['n'] >= 0.95 * R.SIM_SITES
    assert planted['p_mod'] >= planted['p_rep']
    assert 0.2 <= planted['p_rep'] <= 0.8
    if rho > 0.0:
        assert null['p_mod'] < null['p_cond']
    for r, key in ((null, (name, False)), (planted, (name, True))):
        assert (round(r['p_cond'], 4), round(r['p_rep'], 4), round(r['p_mod'], 4)) == REF_RATES[key], (key, r)


def test_the_header_and_the_profile_record_the_measured_rates_and_gates():
    text, prof = open(HEADER).read(), open(PROFILE).read()
    for (name, planted), (pc, pr, pm) in REF_RATES.items():
        k = name.split()[0].replace('v', ' v ')
        line = '%s, rho %s, %s p_cond %.3f  p_rep %.3f  moderated %.3f' % (k, name.split()[-1], 'planted:' if planted else 'null:   ',
                                                                              float('%.3f' % (pc + 1e-9)), float('%.3f' % (pr + 1e-9)), float('%.3f' % (pm + 1e-9)))
        assert line in text, line
        assert '%s p_cond %.4f  p_rep %.4f  moderated %.4f' % ('planted' if planted else 'null   ', pc, pr, pm) in prof, (name, planted)
    for table in (M.MEASURED, M.DEVICE_MEASURED):
        for name, v in table.items():
            assert '%s %.1e' % (name, v) in prof, (name, v)
    assert 'Speed: not measured' in prof
