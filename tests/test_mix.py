"""nmod_mix_fraction (K8) without a GPU: the declaration, the argument checks (before any device work), the error plumbing of the
Python layers, the conditioning of the definition on the inputs the GPU parity test uses (fp64 numpy against 40-digit mpmath),
its statistical sanity on planted mixtures, the command line and the table writer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mix_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def _call(lib, L, npos=4, n=8, *, sig=True, off=True, stride=0, mix_group=1, model=0, max_iter=200, tol=1e-6, out=True, prm=None,
          dtype=None, memspace=None, keep=[]):
    x = np.linspace(-1.0, 1.0, max(npos, 1) * n).astype(np.float32)
    o = np.arange(0, (max(npos, 0) + 1) * n, n, dtype=np.int64)
    res = np.empty(max(npos, 1))
    mo = L.NmodMixOut()
    mo.pi = res.ctypes.data
    keep[:] = [x, o, res]
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_F32 if dtype is None else dtype, stride0=stride, stride1=stride)
    p = lambda a, on: a.ctypes.data_as(C.c_void_p) if on else None
    return lib.nmod_mix_fraction(C.byref(prm), npos, p(x, sig), p(o, off), p(x, sig), p(o, off), mix_group, model, max_iter, tol,
                                 None, 0.05, C.byref(mo) if out else None)


def test_mix_fraction_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_mix_fraction' in set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    assert 'nmod_mix_fraction' in L._SIGNATURES and hasattr(lib, 'nmod_mix_fraction')
    assert 'NMOD_MIX_EQUAL_VAR = 0' in header and 'NMOD_MIX_FREE_VAR = 1' in header
    for name, bit in (('NOT_CONVERGED', 1), ('DEGENERATE', 2), ('SKIPPED', 4), ('VAR_FLOORED', 8), ('TOO_LARGE', 16)):
        assert 'NMOD_MIX_%s = %d' % (name, bit) in header and getattr(L, 'MIX_' + name) == bit == getattr(M, name)
    assert (L.MIX_EQUAL_VAR, L.MIX_FREE_VAR) == (0, 1) == (M.EQUAL, M.FREE) and C.sizeof(L.NmodMixOut) == 56
    assert 'no p-value' in header                            # llr is documented as a score
    assert lib.nmod_abi_version() == 4                       # a purely additive entry


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone would be NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5
    assert _call(lib, L, off=False, stride=8) == -5 and _call(lib, L, model=1, mix_group=0, max_iter=10000, tol=0.0) == -5
    assert _call(lib, L, dtype=L.DTYPE_I16_MILLI) == -5 and _call(lib, L, dtype=L.DTYPE_F64) == -5
    assert _call(lib, L, npos=-1) == -1
    for g in (-1, 2):
        assert _call(lib, L, mix_group=g) == -1
    for m in (-1, 2):
        assert _call(lib, L, model=m) == -1
    for it in (0, -5, 10001):
        assert _call(lib, L, max_iter=it) == -1
    for tol in (-1e-9, float('nan'), float('inf')):
        assert _call(lib, L, tol=tol) == -1, tol
    assert _call(lib, L, out=False) == -1
    assert _call(lib, L, sig=False) == -1                                       # NULL signals with npos > 0
    assert _call(lib, L, off=False) == -1                                       # neither offsets nor a stride
    assert _call(lib, L, dtype=7) == -1 and _call(lib, L, memspace=5) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, prm=bad) == -1
    assert lib.nmod_mix_fraction(None, 4, None, None, None, None, 1, 0, 200, 1e-6, None, 0.05, None) == -1
    # npos == 0 needs no device, no signals and no offsets
    assert _call(lib, L, npos=0) == 0 and _call(lib, L, npos=0, sig=False, off=False) == 0
    assert b'no HIP device' in lib.nmod_strerror(-5)


def test_python_layers_raise():
    import nanomod_amd as nm
    from nanomod_amd import detect, engine
    L = nm._lib
    x = np.linspace(-1.0, 1.0, 40).astype(np.float32)
    off = np.arange(0, 41, 10, dtype=np.int64)
    with pytest.raises(L.NanomodLibraryError, match='nmod_mix_fraction failed: no HIP device'):
        engine.mix_fraction_host(x, off, x, off, device=NO_SUCH_DEVICE)
    with pytest.raises(L.NanomodLibraryError, match='nmod_mix_fraction'):
        engine.mix_fraction_host(x, None, x, None, stride0=10, stride1=10, model='free', mix_group=0, want_resp=True, device=NO_SUCH_DEVICE)
    for kw in (dict(model='storey'), dict(model=2), dict(mix_group=2), dict(mix_group=-1), dict(max_iter=0), dict(max_iter=10001),
               dict(max_iter=2.5), dict(tol=-1.0), dict(tol=float('nan')), dict(tol=float('inf'))):
        with pytest.raises(ValueError):
            engine.mix_fraction_host(x, off, x, off, device=NO_SUCH_DEVICE, **kw)
    with pytest.raises(ValueError, match='gate'):
        engine.mix_fraction_host(x, off, x, off, gate=np.zeros(3), device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.mix_fraction_host(x, off, x.astype(np.float64), off, device=NO_SUCH_DEVICE)
    empty = engine.mix_fraction_host(x[:0], np.zeros(1, np.int64), x[:0], np.zeros(1, np.int64), want_resp=True, device=NO_SUCH_DEVICE)
    assert sorted(empty) == ['iters', 'llr', 'mu_mod', 'pi', 'resp', 'sd_mod', 'status'] and all(a.size == 0 for a in empty.values())
    with pytest.raises(L.NanomodLibraryError, match='nmod_mix_fraction'):
        detect.mix_tracks(x, off, x, off, 'equal', device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError, match='nmod_mix_group'):
        detect.mix_tracks(x, off, x, off, 'equal', group=0, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError, match='nmod_mix'):
        detect._mix_option({'nmod_mix': 'storey'})
    assert detect._mix_option({}) == '' and detect._mix_option({'nmod_mix': 'free'}) == 'free'
    assert callable(nm.DeviceDetector.mix) and 'gate=q' in nm.DeviceDetector.mix.__doc__


def _pin(model):
    """worst fp64-vs-mpmath error over the parity inputs at the oracle's own iteration counts (max_iter 50: what the null
    positions of the GPU test run), in units of the gates: relative (pi, sd_mod), s (mu_mod), relative + absolute (llr)"""
    import mpmath as mp
    ref_rows, mix_rows = M.parity_inputs()
    worst = dict(pi=0.0, mu_mod=0.0, sd_mod=0.0, llr=0.0)
    for x, y in zip(ref_rows, mix_rows):
        own = M.run(x, y, model, max_iter=50, tol=1e-6)
        assert own['status'] & M.DEGENERATE == 0
        a, b = M.em(x, y, model, own['iters']), M.em_mp(x, y, model, own['iters'])
        with mp.workdps(40):
            worst['pi'] = max(worst['pi'], float(abs(a['pi'] - b['pi']) / b['pi']))
            worst['sd_mod'] = max(worst['sd_mod'], float(abs(a['sd_mod'] - b['sd_mod']) / b['sd_mod']))
            worst['mu_mod'] = max(worst['mu_mod'], float(abs(a['mu_mod'] - b['mu_mod']) / b['s']))
            worst['llr'] = max(worst['llr'], float(abs(a['llr'] - b['llr']) / (abs(b['llr']) + 1)))
    return worst


@pytest.mark.parametrize('model', [M.EQUAL, M.FREE])
def test_conditioning_pin(model):
    """The inputs of the GPU parity test can be gated at 1e-9: fp64 numpy and 40-digit mpmath agree to <= 1e-11 at equal iteration
    counts (llr: 1e-11 relative + 1e-11 absolute, checked as |a - b| <= 1e-11 (|b| + 1)).  Measured here: equal variance pi 1.2e-15,
    mu_mod 2.7e-15 s, llr 3.4e-13; free variance pi 1.8e-15, mu_mod 2.4e-15 s, sd_mod 1.1e-15, llr 1.8e-13 — no position of the set
    had to be dropped for either model."""
    worst = _pin(model)
    print('conditioning pin, model %d: %r' % (model, worst))
    assert all(w <= 1e-11 for w in worst.values()), worst


@pytest.mark.parametrize('frac', [0.1, 0.3, 0.6])
def test_planted_mixtures_are_recovered(frac):
    """Planted mixtures, shift 3 sigma, 400 v 400, 200 positions per fraction, equal-variance model with the defaults: the median
    estimated pi lies within 0.03 of the planted fraction, and the median posterior of the planted reads exceeds that of the
    unplanted ones by more than 0.5.  The oracle's own results (this file, seed below): median pi 0.1009 / 0.2997 / 0.5989 for
    0.1 / 0.3 / 0.6, median resp gap 0.915 / 0.970 / 0.977 — the issue's bound of 0.03 stays as it is."""
    rng = np.random.default_rng(int(frac * 1000) + 7)
    pis, gaps = [], []
    for _ in range(200):
        x, y, planted = M.planted_rows(rng, 400, 400, frac, 3.0)
        r = M.run(x, y, M.EQUAL)
        assert r['status'] & M.DEGENERATE == 0
        pis.append(r['pi'])
        gaps.append(np.median(r['resp'][planted]) - np.median(r['resp'][~planted]))
    print('planted %.1f: median pi %.4f, median resp gap %.3f' % (frac, np.median(pis), np.median(gaps)))
    assert abs(np.median(pis) - frac) <= 0.03
    assert np.median(gaps) > 0.5


def test_oracle_statuses_and_stopping_rule():
    rng = np.random.default_rng(3)
    x, y, _ = M.planted_rows(rng, 200, 200, 0.4, 4.0)
    full = M.run(x, y, M.FREE, max_iter=200, tol=1e-8)
    assert 0 < full['iters'] < 200 and full['status'] & M.NOT_CONVERGED == 0 and full['delta'] <= 1e-8 < full['delta_prev']
    same = M.em(x, y, M.FREE, full['iters'])
    assert all(same[k] == full[k] for k in M.FIELDS) and same['delta'] == full['delta']
    capped = M.run(x, y, M.FREE, max_iter=3, tol=1e-8)
    assert capped['iters'] == 3 and capped['status'] & M.NOT_CONVERGED
    assert M.run(x, y, M.EQUAL, max_iter=40, tol=0.0)['iters'] == 40                     # tol = 0 never stops early
    for xx, yy in ((x[:1], y), (x, y[:1]), (np.full(9, 7, np.int16), y), (np.r_[M.as_double(x), np.nan], M.as_double(y))):
        d = M.run(xx, yy, M.EQUAL)
        assert d['status'] == M.DEGENERATE and d['iters'] == 0 and np.isnan(d['pi']) and np.isnan(d['resp']).all()
    # all of Y equal to mu: t_i = 0, r_i = 1/2, the parameters reproduce themselves: converged after one iteration, llr = 0
    flat = M.run(np.array([1.0, 3.0]), np.full(6, 2.0), M.EQUAL)
    assert (flat['pi'], flat['mu_mod'], flat['iters'], flat['status']) == (0.5, 2.0, 1, 0) and abs(flat['llr']) < 1e-15
    # a tight cluster inside a wide reference group: the free variance hits its floor
    tight = M.run(np.linspace(-1.0, 1.0, 50), np.r_[np.full(30, 0.4), np.full(30, 0.401)], M.FREE)
    assert tight['status'] & M.VAR_FLOORED and tight['sd_mod'] == np.sqrt(np.var(np.linspace(-1.0, 1.0, 50)) / 16.0)


def test_cli_lists_the_flags_and_nmod_options_carries_them(capsys):
    from nanomod_amd import cli
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        parser.parse_args(['detect', '--help'])
    text = capsys.readouterr().out
    assert '--mixFraction {none,equal,free}' in text and '--mixGroup {1,2}' in text and '--mixMaxIter' in text and '--mixTol' in text
    base = ['detect', '--wrkBase1', 'a', '--wrkBase2', 'b']
    o = cli.nmod_options(parser.parse_args(base))
    assert (o['nmod_mix'], o['nmod_mix_group'], o['nmod_mix_max_iter'], o['nmod_mix_tol']) == ('', 2, 200, 1e-6)
    o = cli.nmod_options(parser.parse_args(base + ['--mixFraction', 'free', '--mixGroup', '1', '--mixMaxIter', '50', '--mixTol', '1e-8']))
    assert (o['nmod_mix'], o['nmod_mix_group'], o['nmod_mix_max_iter'], o['nmod_mix_tol']) == ('free', 1, 50, 1e-8)
    assert cli.nmod_options(parser.parse_args(base + ['--mixFraction', 'none']))['nmod_mix'] == ''
    for bad in (['--mixFraction', 'three'], ['--mixGroup', '3']):
        with pytest.raises(SystemExit):
            parser.parse_args(base + bad)
    a = parser.parse_args(base + ['--mixMaxIter', '0', '--mixTol', '-1'])
    errs = cli.validate(a)
    assert any('--mixMaxIter' in e for e in errs) and any('--mixTol' in e for e in errs)


def _records():
    recs = []
    for i, (c, s) in enumerate((('chrA', '+'), ('chrB', '-'), ('chrB', '-'))):
        stats = [(10.0 + i, 0.5), (0.25, 0.125), (0.5, 1e-3), (1.5, 2e-4)]
        recs.append(((c, s, 9 + i, 'ACG'[i], 20, 30), stats))
    return recs


def test_mix_table_writer_and_option_off_invariance(tmp_path, capsys):
    """save_test (host-only: the table writer needs no device) with the option off writes what it wrote before, whatever else
    moptions holds; with it on, the mix table beside the unchanged sign-test table"""
    from nanomod_amd import detect
    mix = dict(pi=np.array([0.25, np.nan, 0.5]), mu_mod=np.array([1.5, np.nan, -2.0]), sd_mod=np.array([0.2, np.nan, 0.125]),
               llr=np.array([123.4567, np.nan, 0.0]), iters=np.array([12, 0, 200], np.int32), status=np.array([0, 4, 9], np.uint8))

    def save(folder, **extra):
        os.makedirs(folder)
        mo = dict(SaveTest=1, outFolder=str(folder), FileID='x', neighborPvalues=2, testMethod='stouffer', outLevel=3, mstd=0,
                  sign_test=_records(), **extra)
        keys = set(mo)
        detect.save_test(mo)
        assert set(mo) == keys
        return sorted(os.listdir(folder)), open(os.path.join(folder, 'x_sign_test.txt')).read(), capsys.readouterr().out.replace(str(folder), 'OUT')
    plain = save(tmp_path / 'a')
    assert plain[0] == ['x_sign_test.txt']
    off = save(tmp_path / 'b', sign_test_mix=mix, nmod_mix='')                  # the option off: the array alone writes nothing
    assert off == plain
    on = save(tmp_path / 'c', sign_test_mix=mix, nmod_mix='equal')
    assert on[0] == ['x_sign_test.txt', 'x_sign_test_mix.txt'] and on[1:] == plain[1:]
    got = open(tmp_path / 'c' / 'x_sign_test_mix.txt').read()
    assert got == ('chrA + 10 A 0.250000 1.500000 0.200000 123.457 12 0\n'
                   'chrB - 12 G 0.500000 -2.000000 0.125000 0.000 200 9\n')                # the gated-out position is omitted
    assert [ln.split(' ')[:4] for ln in got.splitlines()] == [ln.split(' ')[:4] for i, ln in enumerate(plain[1].splitlines()) if i != 1]
