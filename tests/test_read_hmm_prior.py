"""CPU: the restatements of the read chain with a per-site prior (K23, tests/hmm_prior_ref.py): against a brute force over all paths and
against mpmath, a constant share against the restatements of K19 - K21, the gradient against central differences of the mpmath
log-likelihood, readllr.site_prior, fit_hmm with the shares held, the declarations, exports and bindings of the three entries, and the
refusals of the Python layer.  Nothing here needs a GPU."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hmm_fit_ref as F
import hmm_prior_ref as P
import hmm_ref as H
import viterbi_ref as V
from nanomod_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARES = np.array([1e-9, 0.02, 0.3, 0.5, 0.97, 1.0 - 1e-9])
ENTRIES = ('nmod_read_hmm_prior', 'nmod_read_viterbi_prior', 'nmod_read_hmm_grad_prior')


def _read(rng, m, shares=SHARES, spread=3.0, gaps=(1, 40)):
    x = np.concatenate(([0], np.cumsum(rng.integers(gaps[0], gaps[1] + 1, m - 1)))).astype(np.float64)
    return x, rng.normal(0.0, spread, m), shares[rng.integers(0, len(shares), m)]


def test_resolve_clamps_and_takes_pi_for_a_nan():
    site_pi = np.array([1e-12, 1e-9, 0.3, 1.0 - 1e-9, 1.0, 0.0, np.nan, np.inf, -np.inf])
    p = P.resolve(site_pi, np.arange(9)[::-1], 0.25)
    assert p.tolist() == [1e-9, 1.0 - 1e-9, 0.25, 1e-9, 1.0 - 1e-9, 1.0 - 1e-9, 0.3, 1e-9, 1e-9]


@pytest.mark.parametrize('m', range(1, 11))
def test_the_restatements_agree_with_all_paths(m):
    """posterior, ll, the best path, vit and delta from the 2^m paths' joint probabilities (float64: compared at 1e-9, far above its own
    rounding and far below any error of the model) against the sequential restatements and those in the device's order"""
    rng = np.random.default_rng(2300 + m)
    for length in (3.0, 40.0, 1e4):
        x, s, p = _read(rng, m)
        bf = P.brute_force(x, s, p, length)
        for hmm, vit in ((P.hmm_seq, P.viterbi_seq), (P.hmm_device_order, P.viterbi_device_order)):
            h, v = hmm(x, s, p, length), vit(x, s, p, length)
            assert np.allclose(h['post'], bf['post'], rtol=1e-9, atol=1e-300) and abs(h['ll'] - bf['ll']) <= 1e-9 * (abs(bf['ll']) + 1.0)
            assert abs(v['vit'] - bf['vit']) <= 1e-9 * (abs(bf['vit']) + 1.0)
            assert np.allclose(v['delta'], bf['delta'], rtol=1e-9, atol=1e-9)
            if m == 1 or bf['vit'] - bf['second'] > 1e-9:                      # (the best path is the only one)
                assert v['path'].tolist() == bf['path'].tolist()
            assert np.all((v['delta'] > 0) == (v['path'] == 1)) or np.any(np.abs(v['delta']) < 1e-9)


@pytest.mark.parametrize('m', [1, 2, 7, 65, 300, 1100])
def test_the_restatements_lie_within_their_gates_of_mpmath(m):
    import mpmath as mp
    rng = np.random.default_rng(2320 + m)
    x, s, p = _read(rng, m)
    length = 25.0
    ex = P.chain_mp(x, s, p, length)
    g = P.gate(m)
    for hmm, grad, vit in ((P.hmm_seq, P.grad_seq, P.viterbi_seq), (P.hmm_device_order, P.grad_device_order, P.viterbi_device_order)):
        h, gr, v = hmm(x, s, p, length), grad(x, s, p, length), vit(x, s, p, length)
        for j in range(m):
            assert abs(mp.mpf(float(h['post'][j])) - ex['post'][j]) <= g * ex['post'][j] + mp.mpf(H.FLOOR), j
        for f in ('ll', 'll_indep'):
            assert abs(mp.mpf(h[f]) - ex[f]) <= g * (ex['denom'] + 1), f
        assert gr['ll'] == h['ll'] or hmm is P.hmm_seq
        assert abs(mp.mpf(gr['g_eta']) - ex['g_eta']) <= P.gate_eta(m) * (ex['abs_eta'] + 1)
        assert abs(mp.mpf(gr['g_lam']) - ex['g_lam']) <= P.gate_lam(m) * (ex['abs_lam'] + 1)
        gv = P.gate_vit(m) * (P.vit_scale(x, s, p, length) + 1.0)
        exv = P.viterbi_mp(x, s, p, length, gv)
        assert abs(mp.mpf(v['vit']) - exv['vit']) <= gv and np.all(np.abs(v['delta'] - exv['delta']) <= gv)
        sure = np.abs(exv['delta']) > gv + exv['near_loss']
        assert sure.mean() > 0.9 and np.array_equal(v['path'][sure], exv['path'][sure])
        assert abs(exv['scale'] - P.vit_scale(x, s, p, length)) <= 1e-9 * exv['scale']


@pytest.mark.parametrize('m', [1, 2, 9, 70, 1030])
def test_a_constant_share_is_the_plain_chain(m):
    """the same operations on the same doubles: exact, but g_eta, whose product is made per term and not on the sum (within its gate)"""
    rng = np.random.default_rng(2340 + m)
    for pi in (0.3, 1e-9, 1.0 - 1e-9):
        x, s, _ = _read(rng, m)
        p = np.full(m, pi)
        for mine, plain in ((P.hmm_seq, H.hmm_seq), (P.hmm_device_order, H.hmm_device_order)):
            a, b = mine(x, s, p, 30.0), plain(x, s, pi, 30.0)
            assert np.array_equal(a['post'], b['post']) and a['ll'] == b['ll'] and a['ll_indep'] == b['ll_indep']
        for mine, plain in ((P.viterbi_seq, V.viterbi_seq), (P.viterbi_device_order, V.viterbi_device_order)):
            a, b = mine(x, s, p, 30.0), plain(x, s, pi, 30.0)
            assert np.array_equal(a['path'], b['path']) and a['vit'] == b['vit'] and np.array_equal(a['delta'], b['delta'])
        assert P.vit_scale(x, s, p, 30.0) == V.scale(x, s, pi, 30.0)
        for mine, plain in ((P.grad_seq, F.grad_seq), (P.grad_device_order, F.grad_device_order)):
            a, b = mine(x, s, p, 30.0), plain(x, s, pi, 30.0)
            assert a['ll'] == b['ll'] and a['g_lam'] == b['g_lam'] and a['abs_lam'] == b['abs_lam']
            assert F.within(a['g_eta'], b['g_eta'], P.gate_eta(m), b['abs_eta']) and F.within(a['abs_eta'], b['abs_eta'], P.gate_eta(m), b['abs_eta'])


def test_the_gates_add_what_the_docstring_says():
    for m in (1, 5, 64, 1024, 1025, 5000):
        assert P.gate(m) == H.gate(m) and P.gate_lam(m) == F.gate_lam(m)
        assert V.gate(m) <= P.gate_vit(m) <= V.gate(m) + 4 * P.U + 1e-30 and F.gate_eta(m) <= P.gate_eta(m) <= F.gate_eta(m) + P.U + 1e-30
    assert P.gate_vit(1) == P.U * (2 * (38 + 4 + 2 + V.path_v(1)) + (4 + 8 + 1) + 6)


@pytest.mark.parametrize('m', [2, 6, 40])
def test_the_gradient_is_the_derivative_of_the_mpmath_log_likelihood(m):
    """central differences at 60 digits: in ln(length), and in a common offset kappa of the logits of all shares (q = 1 - pi exactly)"""
    import mpmath as mp
    rng = np.random.default_rng(2360 + m)
    x, s, p = _read(rng, m, shares=np.array([0.02, 0.3, 0.5, 0.97, 0.11]))
    length = 35.0
    ex = P.chain_mp(x, s, p, length)
    with mp.workdps(60):
        h = mp.mpf(10) ** -20
        pm = [mp.mpf(float(v)) for v in p]

        def at(kappa, lam):
            sh = [1 / (1 + mp.exp(-(mp.log(v) - mp.log(1 - v) + kappa))) for v in pm]
            return P.ll_mp(x, s, sh, [1 - v for v in sh], mp.exp(lam))
        lam0 = mp.log(mp.mpf(length))
        d_eta = (at(h, lam0) - at(-h, lam0)) / (2 * h)
        d_lam = (at(0, lam0 + h) - at(0, lam0 - h)) / (2 * h)
        # (the restatement takes q_j as the double 1.0 - p_j: u relative to q, far below 1e-12 of the terms' sum)
        assert abs(d_eta - ex['g_eta']) <= mp.mpf(10) ** -12 * (ex['abs_eta'] + 1)
        assert abs(d_lam - ex['g_lam']) <= mp.mpf(10) ** -12 * (ex['abs_lam'] + 1)
        assert abs(at(0, lam0) - ex['ll']) <= mp.mpf(10) ** -12 * (abs(ex['ll']) + 1)


def test_site_prior_arithmetic_and_refusals():
    from nanomod_amd import readllr
    pi_hat = np.array([0.0, 1.0, np.nan, 0.5, 0.25])
    n = np.array([2, 3, 0, 10, 0])
    got = readllr.site_prior(pi_hat, n, 0.3, 4.0)
    want = [(2 * 0.0 + 4.0 * 0.3) / 6.0, (3 * 1.0 + 4.0 * 0.3) / 7.0, math.nan, (10 * 0.5 + 4.0 * 0.3) / 14.0, 0.3]
    assert got.dtype == np.float64 and np.array_equal(got, np.array(want), equal_nan=True)
    assert 0.0 < got[0] < got[1] < 1.0                                         # a hard 0 or 1 from a few reads does not stay one
    assert len(readllr.site_prior(np.zeros(0), np.zeros(0), 0.5, 1.0)) == 0
    for bad in (dict(mean=0.0), dict(mean=1.0), dict(mean=math.nan), dict(prior_reads=0.0), dict(prior_reads=-1.0), dict(prior_reads=math.nan),
                dict(prior_reads=math.inf), dict(n_valid=np.array([1, -1, 0, 1, 1])), dict(n_valid=np.array([1, 2])), dict(pi_hat=pi_hat + 1.0)):
        with pytest.raises(ValueError):
            readllr.site_prior(**dict(dict(pi_hat=pi_hat, n_valid=n, mean=0.3, prior_reads=4.0), **bad))


def test_fit_hmm_with_the_shares_held_fits_the_length_alone():
    """reads simulated from the model with two kinds of sites, the evaluator the prior restatement at the true shares: fix_pi (what a
    site prior forces) leaves pi where it was, and the fitted length covers the true one"""
    from nanomod_amd import readllr
    rng = np.random.default_rng(2380)
    length, sep = 60.0, 2.5
    reads = []
    for _ in range(150):
        m = int(rng.integers(8, 20))
        x = np.concatenate(([0], np.cumsum(rng.integers(2, 25, m - 1)))).astype(np.float64)
        p = np.where((x // 40) % 2 == 0, 0.08, 0.7)
        z = np.zeros(m, np.int64)
        for j in range(m):
            rho = math.exp(-(x[j] - x[j - 1]) / length) if j else 0.0
            z[j] = z[j - 1] if j and rng.random() < rho else rng.random() < p[j]
        reads.append((x, sep * rng.normal(sep * z, 1.0) - 0.5 * sep * sep, p))
    hoff = np.concatenate(([0], np.cumsum([len(s) for _, s, _ in reads]))).astype(np.int64)

    def evaluate(pi, v):
        res = [P.grad_seq(x, s, p, v) for x, s, p in reads]
        return F.batch_sums([r['ll'] for r in res], [r['g_eta'] for r in res], [r['g_lam'] for r in res], hoff).tolist()
    fit = readllr.fit_hmm(evaluate, 0.3, 200.0, fix_pi=True)
    assert fit['pi'] == 0.3 and fit['converged'] and fit['status'].startswith('length fitted alone: pi is fixed') and math.isnan(fit['se_eta'])
    assert fit['length_lo'] < length < fit['length_hi'] and fit['length'] != 200.0
    flat = readllr.fit_hmm(lambda pi, v: F.evaluator([(x, s) for x, s, _ in reads])(0.3, v), 0.3, 200.0, fix_pi=True)
    assert fit['ll'] > flat['ll']                                              # the sites' own shares explain the reads better than their mean
    with pytest.raises(ValueError, match='fix_pi=False'):
        readllr.smooth_reads_llr(None, None, None, fit='mle', fix_pi=False, site_prior=True)
    with pytest.raises(ValueError, match='prior_reads'):
        readllr.smooth_reads_llr(None, None, None, site_prior=True, prior_reads=0.0)


def test_the_entries_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert '#define NMOD_ABI_VERSION 4' in text and L.NMOD_ABI_VERSION == 4
    lib = L.load()
    assert lib.nmod_abi_version() == 4
    exported = subprocess.check_output(['nm', '-D', '--defined-only', L.LIB_PATH]).decode()
    for name in ENTRIES:
        plain = name[:-len('_prior')]
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, text)
        assert decl and re.search(r'\b%s\b' % name, exported)
        args = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
        want = [a.strip() for a in re.search(r'\bint %s\(([^;]*)\);' % plain, text).group(1).replace('\n', ' ').split(',')]
        assert args == want[:8] + ['const double* site_pi'] + want[8:]         # the counterpart's arguments, site_pi after key
        sig, base = L._SIGNATURES[name][1], L._SIGNATURES[plain][1]
        assert sig == base[:8] + [base[7]] + base[8:] and getattr(lib, name).argtypes is not None
    assert 'CAVEAT' in text and 'rho P(z_(j-1) = 1) + eps pi_j' in text and 'a per-site prior on request: K23' in text
    for unit in ('read_hmm.hip', 'read_viterbi.hip'):
        code = re.sub(r'//.*', '', open(os.path.join(ROOT, 'nanomod_amd', 'csrc', unit)).read())
        assert 'bool PRIOR' in code and 'asm' not in code and not re.search(r'atomicAdd\(\s*\(?\s*(double|float)', code)
    mk = open(os.path.join(ROOT, 'nanomod_amd', 'csrc', 'Makefile')).read()
    assert 'read_hmm.o: CXXFLAGS += -ffp-contract=off' in mk and 'read_viterbi.o: CXXFLAGS += -ffp-contract=off' in mk


def test_the_python_layer_refuses_a_wrong_site_pi_before_any_device_work():
    from nanomod_amd import cli, engine
    key = np.arange(5, dtype=np.int64) + 3
    reads = (np.zeros(2, np.int32), np.zeros(2, np.int64), np.array([0, 4, 9], np.int64), np.zeros(9), key)
    hoff = np.array([0, 1, 2], np.int64)
    for fn in (engine.read_hmm_host, engine.read_viterbi_host, engine.read_hmm_grad_host):
        for bad in (np.zeros(4), np.zeros(6), np.zeros(5, np.float32), np.zeros((5, 1)), [0.5] * 5, 0.5):
            with pytest.raises(ValueError, match='site_pi'):
                fn(*reads, hoff, site_pi=bad, device=99)
    argv = ['readhmm', '--wrkBase1', __file__, '--model', __file__, '--altModel', __file__]
    a = cli.build_parser().parse_args(argv)
    assert a.sitePrior == 0 and a.priorReads == 4.0
    a = cli.build_parser().parse_args(argv + ['--sitePrior', '1', '--priorReads', '0'])
    assert any('--priorReads' in e for e in cli.validate_readhmm(a))
    a = cli.build_parser().parse_args(argv + ['--priorReads', '0'])            # (not read without --sitePrior 1)
    assert not any('--priorReads' in e for e in cli.validate_readhmm(a))
