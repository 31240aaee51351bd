"""CPU: the restatements of nmod_read_hmm_grad (K21, tests/hmm_fit_ref.py): the mpmath gradient against central differences of the
mpmath log-likelihood, the float64 restatements within the derived gates of mpmath, readllr.fit_hmm on the restatement's evaluator (the
simulated sample, the fixed-pi path, the parameters that are not identified), the bindings' layout against the header, the refusals of
the Python layer and the command line, and the writer's format.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import hmm_fit_ref as F
import hmm_ref as H
from nanomod_amd import _lib as L
from nanomod_amd import readllr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
TRUE_PI, TRUE_LENGTH = 0.3, 150.0


def _read(m, seed, kind='normal', max_gap=23):
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(1, max_gap + 1, m)).astype(np.float64)
    if kind == 'zero':
        return x, np.zeros(m)
    if kind == 'extreme':
        return x, rng.choice(np.array([800.0, -800.0, 5.0, -5.0, 0.0, 40.0]), m)
    return x, rng.normal(0.0, 3.0, m)


# ------------------------------------------------------------------------------------------------------------ the definition
@pytest.mark.parametrize('pi,length', [(0.3, 150.0), (1e-9, 1e-3), (1.0 - 1e-9, 1e9), (1e-9, 1e9), (1.0 - 1e-9, 1e-3)])
@pytest.mark.parametrize('m', [1, 2, 3, 5, 40])
def test_the_mpmath_gradient_is_the_derivative_of_the_mpmath_log_likelihood(m, pi, length):
    """Central differences of the 60-digit log-likelihood at a step of 1e-25 in eta and in lam.  hmm_ref.hmm_mp takes its parameters as
    doubles, so the differences are taken of hmm_fit_ref.ll_mp, the same recursion with mpf parameters, which is first shown to be
    hmm_mp's ll at the doubles.  The entry forms q = 1 - pi as a double, so q + pi is 1 only to within 2^-53, and along eta the
    path is pi +- h pi q, q -+ h pi q: its derivative is the header's g_eta plus post_0 (q + pi - 1), which is added here exactly."""
    import mpmath as mp
    x, s = _read(m, 2100 + m)
    exact = F.grad_mp(x, s, pi, length)
    ref = H.hmm_mp(x, s, pi, length)
    with mp.workdps(60):
        p, q, v = mp.mpf(pi), mp.mpf(1.0 - pi), mp.mpf(length)
        assert abs(F.ll_mp(x, s, p, q, v) - ref['ll']) <= mp.mpf(10) ** -50 * (abs(ref['ll']) + 1)
        assert abs(exact['ll'] - ref['ll']) <= mp.mpf(10) ** -50 * (abs(ref['ll']) + 1)
        h = mp.mpf(10) ** -25
        d = h * p * q
        cd_eta = (F.ll_mp(x, s, p + d, q - d, v) - F.ll_mp(x, s, p - d, q + d, v)) / (2 * h)
        cd_lam = (F.ll_mp(x, s, p, q, v * mp.exp(h)) - F.ll_mp(x, s, p, q, v * mp.exp(-h))) / (2 * h)
        err_eta = abs(cd_eta - (exact['g_eta'] + ref['post'][0] * (q + p - 1)))
        err_lam = abs(cd_lam - exact['g_lam'])
        print('m %d pi %g length %g: g_eta %.6g g_lam %.6g, central differences off by %.3g, %.3g' % (m, pi, length, float(exact['g_eta']),
              float(exact['g_lam']), float(err_eta), float(err_lam)))
        assert err_eta <= mp.mpf(10) ** -30 * (exact['abs_eta'] + 1) and err_lam <= mp.mpf(10) ** -30 * (exact['abs_lam'] + 1)
        assert exact['abs_eta'] >= abs(exact['g_eta']) and exact['abs_lam'] >= abs(exact['g_lam'])
        if m == 1:
            assert exact['g_lam'] == 0 and exact['abs_lam'] == 0


CASES = [(1, 'normal', 0.3, 150.0), (2, 'normal', 0.5, 30.0), (2, 'extreme', 1e-9, 1e9), (5, 'normal', 1.0 - 1e-9, 1e-3), (40, 'extreme', 0.3, 150.0),
         (40, 'zero', 0.3, 150.0), (255, 'normal', 0.2, 200.0), (256, 'normal', 0.2, 200.0), (257, 'extreme', 1e-9, 1e9), (H.WAVE_MAX, 'normal', 0.7, 400.0),
         (H.WAVE_MAX + 1, 'normal', 0.3, 150.0), (2500, 'normal', 0.05, 60.0), (2500, 'zero', 0.4, 1e6)]


@pytest.mark.parametrize('m,kind,pi,length', CASES)
def test_both_float64_restatements_against_mpmath_within_the_gates(m, kind, pi, length):
    import mpmath as mp
    x, s = _read(m, 2150 + m, kind)
    exact = F.grad_mp(x, s, pi, length)
    ge, gl = F.gate_eta(m), F.gate_lam(m)
    for name, chain in (('sequential', F.grad_seq), ('device order', F.grad_device_order)):
        res = chain(x, s, pi, length)
        with mp.workdps(60):
            err_e = abs(mp.mpf(res['g_eta']) - exact['g_eta']) / (exact['abs_eta'] + 1)
            err_l = abs(mp.mpf(res['g_lam']) - exact['g_lam']) / (exact['abs_lam'] + 1)
            print('%s m %d: g_eta off by %.3g of abs_eta + 1 (gate %.3g), g_lam by %.3g of abs_lam + 1 (gate %.3g)' % (name, m, float(err_e), ge, float(err_l), gl))
            assert err_e <= ge and err_l <= gl
            for f in ('abs_eta', 'abs_lam'):
                assert abs(mp.mpf(res[f]) - exact[f]) <= max(ge, gl) * (exact[f] + 1)
    assert F.grad_device_order(x, s, pi, length)['ll'] == H.hmm_device_order(x, s, pi, length)['ll']
    assert F.grad_seq(x, s, pi, length)['ll'] == H.hmm_seq(x, s, pi, length)['ll']


def test_the_gates_grow_from_the_roundings_and_are_capped():
    assert F.REL_U == 40 and F.LREL_U == 785 and F.vec_u(1) == 29 * 2 + 2 * 28
    assert F.gate_eta(1) == H.U * (40 + 114 + 1 + 7 + 0 + 2 * 114 + 5) and F.gate_lam(1) == H.U * (785 + 114 + 1 + 7)
    assert F.gate_eta(2) < F.gate_eta(5) < F.gate_eta(15) < H.CAP == F.gate_eta(16) == F.gate_eta(5000)
    assert F.gate_lam(1) < F.gate_lam(2) < H.CAP == F.gate_lam(3) == F.gate_lam(5000)
    assert F.read_grad_ref(np.zeros(1, np.int32), np.zeros(1, np.int64), np.array([0, 3]), np.zeros(3), np.array([7], np.int64), 0.3, 150.0)['status'].tolist() == [1]


def test_the_fixed_order_sums_are_the_plain_sums_in_another_order():
    rng = np.random.default_rng(2104)
    n = 700
    ll, e, v = rng.normal(0, 5, n), rng.normal(0, 2, n), rng.normal(0, 1, n)
    hoff = np.concatenate(([0], np.cumsum(rng.integers(0, 4, n))))
    got = F.batch_sums(ll, e, v, hoff)
    want = [math.fsum(a) for a in (ll, e, v, e * e, e * v, v * v)]
    assert np.allclose(got[:6], want, rtol=0, atol=1e-11) and got[6] == (np.diff(hoff) > 0).sum() and got[7] == hoff[-1]
    assert F.batch_sums([], [], [], [0]).tolist() == [0.0] * 8
    assert F.batch_sums([1.5], [2.0], [-3.0], [0, 4]).tolist() == [1.5, 2.0, -3.0, 4.0, -6.0, 9.0, 1.0, 4.0]


# ------------------------------------------------------------------------------------------------------------ the fit
@pytest.fixture(scope='module')
def sample():
    reads = F.simulate_chain_reads()
    evaluate = F.evaluator(reads)
    return dict(reads=reads, evaluate=evaluate, fit=readllr.fit_hmm(evaluate, 0.5, 200.0))


def test_the_fit_converges_on_the_simulated_sample_and_covers_the_truth(sample):
    fit = sample['fit']
    print('fit: pi %.6f (%.6f .. %.6f), length %.4f (%.4f .. %.4f), %d evaluations' % (fit['pi'], fit['pi_lo'], fit['pi_hi'], fit['length'], fit['length_lo'],
                                                                                        fit['length_hi'], fit['n_eval']))
    assert fit['converged'] and fit['status'] == 'pi and length fitted' and fit['n_eval'] <= 8 and len(fit['trace']) == fit['n_eval']
    assert fit['n_reads'] == len(sample['reads']) == 300 and fit['n_entries'] == sum(len(s) for _, s in sample['reads'])
    lls = [row[2] for row in fit['trace']]
    assert all(b > a for a, b in zip(lls, lls[1:])) and fit['trace'][-1][3] < 1e-10 <= fit['trace'][-2][3] and fit['ll'] == lls[-1]
    assert fit['trace'][0][:2] == (0.5, 200.0) and fit['trace'][-1][:2] == (fit['pi'], fit['length'])
    z_eta = (fit['eta'] - readllr._logit(TRUE_PI)) / fit['se_eta']
    z_lam = (fit['lam'] - math.log(TRUE_LENGTH)) / fit['se_lam']
    print('the truth lies %.2f (logit pi) and %.2f (ln length) standard errors from the estimate' % (z_eta, z_lam))
    assert abs(z_eta) < 3.0 and abs(z_lam) < 3.0
    assert fit['pi_lo'] < TRUE_PI < fit['pi_hi'] and fit['length_lo'] < TRUE_LENGTH < fit['length_hi']
    z = 1.959963984540054
    assert math.isclose(fit['pi_hi'], readllr._expit(fit['eta'] + z * fit['se_eta']), rel_tol=1e-12)
    assert math.isclose(fit['length_lo'], math.exp(fit['lam'] - z * fit['se_lam']), rel_tol=1e-12)
    wide = readllr.fit_hmm(lambda p, v: sample['evaluate'](fit['pi'], fit['length']), fit['pi'], fit['length'], ci_level=0.99)
    assert wide['n_eval'] == 1 and wide['converged'] and wide['pi_lo'] < fit['pi_lo'] and wide['length_hi'] > fit['length_hi']


def test_the_fitted_length_beats_every_length_of_a_grid_at_the_fitted_pi(sample):
    fit = sample['fit']
    for v in (12.5, 25.0, 50.0, 100.0, 150.0, 200.0, 400.0, 1600.0):
        assert sample['evaluate'](fit['pi'], v)[0] < fit['ll'], v
    for v in (fit['length'] * 0.98, fit['length'] * 1.02):
        assert sample['evaluate'](fit['pi'], v)[0] < fit['ll'], v


def test_a_fixed_pi_fits_the_length_alone(sample):
    fit = readllr.fit_hmm(sample['evaluate'], TRUE_PI, 400.0, fix_pi=True)
    assert fit['converged'] and fit['pi'] == TRUE_PI and fit['status'] == 'length fitted alone: pi is fixed'
    assert math.isnan(fit['se_eta']) and fit['pi_lo'] == fit['pi_hi'] == TRUE_PI and fit['se_lam'] > 0.0
    assert all(row[0] == TRUE_PI for row in fit['trace']) and abs(fit['lam'] - math.log(TRUE_LENGTH)) < 3.0 * fit['se_lam']
    assert abs(sample['evaluate'](TRUE_PI, fit['length'])[2]) < 1e-3 * math.sqrt(sample['evaluate'](TRUE_PI, fit['length'])[5])


def test_what_is_not_identified_is_not_fitted():
    single = [(x[:1], s[:1]) for x, s in F.simulate_chain_reads(n_reads=80)]
    fit = readllr.fit_hmm(F.evaluator(single), 0.5, 200.0)
    assert fit['converged'] and fit['length'] == 200.0 and fit['status'].startswith('pi fitted alone: no read has two entries')
    assert math.isnan(fit['se_lam']) and fit['length_lo'] == fit['length_hi'] == 200.0 and 0.05 < fit['pi'] < 0.6 and fit['se_eta'] > 0.0
    assert fit['n_reads'] == fit['n_entries'] == 80
    fixed = readllr.fit_hmm(F.evaluator(single), 0.5, 200.0, fix_pi=True)
    assert not fixed['converged'] and fixed['n_eval'] == 1 and fixed['status'].startswith('nothing fitted') and (fixed['pi'], fixed['length']) == (0.5, 200.0)
    none = readllr.fit_hmm(F.evaluator([]), 0.25, 80.0)
    assert not none['converged'] and none['n_eval'] == 1 and none['status'] == 'nothing fitted: no read has an entry' and none['n_reads'] == 0
    assert (none['pi'], none['length'], none['ll']) == (0.25, 80.0, 0.0) and math.isnan(none['se_eta']) and math.isnan(none['se_lam'])
    assert len(none['trace']) == 1


def test_a_step_is_halved_and_the_ranges_hold():
    """a one-parameter likelihood in lam with its maximum at ln 50, handed over as sums: a gradient overstated four times makes the first
    full steps overshoot; and a likelihood that rises for ever stops at the range's end"""
    def peak(pi, length):
        d = math.log(length) - math.log(50.0)
        return [-d * d, 0.0, -8.0 * d, 0.0, 0.0, 4.0, 10.0, 20.0]
    fit = readllr.fit_hmm(peak, 0.3, 400.0, fix_pi=True, tol=1e-12)
    assert fit['converged'] and abs(fit['length'] - 50.0) < 1e-3 and fit['n_eval'] > len(fit['trace'])
    rising = readllr.fit_hmm(lambda pi, length: [math.log(length), 0.0, 1.0, 0.0, 0.0, 1e-4, 10.0, 20.0], 0.3, 400.0, fix_pi=True)
    assert not rising['converged'] and rising['length'] == 1e9 and 'no step increases' in rising['status']
    for bad in (dict(pi0=0.0), dict(length0=1e10), dict(tol=0.0), dict(max_iter=0), dict(ci_level=1.0)):
        kw = dict(dict(pi0=0.3, length0=100.0, tol=1e-10, max_iter=50, ci_level=0.95), **bad)
        with pytest.raises(ValueError):
            readllr.fit_hmm(peak, kw.pop('pi0'), kw.pop('length0'), **kw)
    with pytest.raises(ValueError):
        readllr.fit_hmm(lambda pi, length: [0.0] * 6, 0.3, 100.0)


# ------------------------------------------------------------------------------------------------------------ bindings, refusals, writer
def test_header_bindings_and_build_rule():
    text = open(HEADER).read()
    m = re.search(r'typedef struct nmod_hmm_grad_out \{([^}]*)\} nmod_hmm_grad_out;', text)
    names = re.findall(r'\*\s*(\w+)', re.sub(r'/\*.*?\*/', '', m.group(1)))
    assert tuple(names) == L.HMM_GRAD_READ_FIELDS + ('sums',) == tuple(n for n, _ in L.NmodHmmGradOut._fields_[2:])
    assert 'typedef struct nmod_hmm_grad_opts { int32_t struct_size, reserved; double pi, length; } nmod_hmm_grad_opts;' in text
    assert [n for n, _ in L.NmodHmmGradOpts._fields_] == ['struct_size', 'reserved', 'pi', 'length'] and len(L.HMM_GRAD_SUMS) == 8
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu", sizeof(nmod_hmm_grad_opts), ' \
          'offsetof(nmod_hmm_grad_opts, length), sizeof(nmod_hmm_grad_out), offsetof(nmod_hmm_grad_out, ll), offsetof(nmod_hmm_grad_out, status), ' \
          'offsetof(nmod_hmm_grad_out, sums));return 0;}' % HEADER
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == [C.sizeof(L.NmodHmmGradOpts), L.NmodHmmGradOpts.length.offset, C.sizeof(L.NmodHmmGradOut), L.NmodHmmGradOut.ll.offset,
                   L.NmodHmmGradOut.status.offset, L.NmodHmmGradOut.sums.offset] == [24, 16, 64, 8, 48, 56]
    lib = L.load()
    assert 'nmod_read_hmm_grad' in L._SIGNATURES and lib.nmod_read_hmm_grad.argtypes is not None
    assert len(L._SIGNATURES['nmod_read_hmm_grad'][1]) == len(L._SIGNATURES['nmod_read_hmm'][1])
    src = open(os.path.join(ROOT, 'nanomod_amd', 'csrc', 'read_hmm.hip')).read()
    code = re.sub(r'//.*', '', src)
    assert 'rh_grad_kernel' in code and 'rh_grad_sums_kernel' in code and code.count('struct Mat2') == 1 and code.count('rh_tile(') == 1
    assert not re.search(r'atomicAdd\(\s*\(?\s*(double|float)', code)          # (the unit's rule on contraction: test_read_hmm.py)
    assert 'nmod_read_hmm_grad, below' in text                                  # K19's and K20's "no Baum-Welch" point to it


def test_the_python_layer_refuses_what_the_entry_refuses():
    from nanomod_amd import cli, engine
    for kw in (dict(pi=0.0), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=2e9), dict(length=float('inf')), dict(want=('ll', 'post'))):
        with pytest.raises(ValueError):
            engine._hmm_grad_opts(*[dict(dict(pi=0.3, length=200.0, want=()), **kw)[k] for k in ('pi', 'length', 'want')])
    opts, want = engine._hmm_grad_opts(0.25, 80.0, ('sums', 'll'))
    assert (opts.pi, opts.length, opts.struct_size, want) == (0.25, 80.0, 24, ('sums', 'll'))
    assert list(engine._hmm_grad_shapes(('sums', 'status', 'g_lam'), 7).items()) == [('g_lam', ('float64', 7)), ('status', ('uint8', 7)), ('sums', ('float64', 8))]
    # smooth_reads_llr refuses before it touches the reads or the device
    for kw in (dict(fit='em'), dict(fit='mle', fit_length=[50.0]), dict(fix_pi=True)):
        with pytest.raises(ValueError):
            readllr.smooth_reads_llr(None, None, None, **kw)
    base = ['readhmm', '--wrkBase1', HEADER, '--model', HEADER, '--altModel', HEADER]
    errs = cli.validate_readhmm(cli.build_parser().parse_args(base + ['--fitHmm', '1', '--fitLength', '50,100']))
    assert len(errs) == 1 and '--fitHmm' in errs[0] and '--fitLength' in errs[0]
    errs = cli.validate_readhmm(cli.build_parser().parse_args(base + ['--fixPi', '1']))
    assert len(errs) == 1 and '--fixPi' in errs[0]
    ok = cli.build_parser().parse_args(base + ['--fitHmm', '1', '--fixPi', '1'])
    assert (ok.fitHmm, ok.fixPi) == (1, 1) and not [e for e in cli.validate_readhmm(ok) if 'fit' in e or 'fix' in e]
    plain = cli.build_parser().parse_args(base)
    assert (plain.fitHmm, plain.fixPi) == (0, 0)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ['--fitHmm', '2'])


def test_the_writer_s_format():
    fit = dict(pi=0.3125, length=170.5, eta=-0.79, lam=5.14, ll=2272.25, se_eta=0.106, se_lam=float('nan'), pi_lo=0.25, pi_hi=0.375, length_lo=170.5,
               length_hi=170.5, trace=[(0.5, 200.0, 2242.875, 57.25), (0.3125, 170.5, 2272.25, 6.25e-12)], n_eval=3, n_reads=300, n_entries=4507,
               converged=True, status='pi fitted alone: no read has two entries, length is not identified', ci_level=0.95)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'run_hmm_fit.txt')
        readllr.write_hmm_fit(path, fit)
        assert open(path).read() == ('0 0.5 200 2242.875000 5.725E+01\n1 0.3125 170.5 2272.250000 6.250E-12\n'
                                     'pi 0.3125 0.25 0.375 0.106\nlength 170.5 170.5 170.5 nan\n'
                                     'evaluations 3 converged 1 level 0.95\n'
                                     'status pi fitted alone: no read has two entries, length is not identified\n')
