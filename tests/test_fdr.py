"""nmod_fdr_adjust without a GPU: the declaration, the argument checks (before any device work), the error plumbing of the
Python layers, the command line, and the numpy restatement of the definition against scipy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fdr_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def _call(lib, L, n, tracks, method=0, alpha=0.05, ntracks=None, device=NO_SUCH_DEVICE, memspace=None, null_arrays=False, prm=None):
    nt = len(tracks) if ntracks is None else ntracks
    parr = (C.c_void_p * 8)(*[t.ctypes.data if t is not None else None for t in tracks])
    qarr = (C.c_void_p * 8)(*[t.ctypes.data if t is not None else None for t in tracks])
    if prm is None:
        prm = L.make_params(device=device, memspace=L.MEM_HOST if memspace is None else memspace)
    return lib.nmod_fdr_adjust(C.byref(prm), n, nt, None if null_arrays else parr, method, alpha, None if null_arrays else qarr, None)


def test_fdr_adjust_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_fdr_adjust' in set(re.findall(r'\b(nmod_[a-z0-9_]+)\s*\(', header))
    assert 'nmod_fdr_adjust' in L._SIGNATURES and hasattr(lib, 'nmod_fdr_adjust')
    assert 'NMOD_FDR_BH = 0' in header and 'NMOD_FDR_BY = 1' in header
    assert (L.FDR_BH, L.FDR_BY) == (0, 1) and C.sizeof(L.NmodFdrSummary) == 32
    assert lib.nmod_abi_version() == 4                       # a purely additive entry


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone would be NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    p = np.linspace(0.0, 1.0, 16)
    assert _call(lib, L, 16, [p]) == -5                                        # the well-formed call reaches the device check
    assert _call(lib, L, -1, [p]) == -1
    assert _call(lib, L, 2 ** 31 - 1, [p]) == -1                               # beyond the sort's index range (2^31 - 2)
    assert _call(lib, L, 16, [p], ntracks=0) == -1
    assert _call(lib, L, 16, [p] * 8, ntracks=9) == -1
    assert _call(lib, L, 16, [p, None]) == -1                                  # a NULL track
    assert _call(lib, L, 16, [p], null_arrays=True) == -1
    assert _call(lib, L, 16, [p], method=2) == -1 and _call(lib, L, 16, [p], method=-1) == -1
    for alpha in (0.0, -0.1, 1.0000001, float('nan'), float('inf')):
        assert _call(lib, L, 16, [p], alpha=alpha) == -1, alpha
    assert _call(lib, L, 16, [p], alpha=1.0) == -5 and _call(lib, L, 16, [p], method=1) == -5
    assert _call(lib, L, 16, [p] * 8) == -5
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, 16, [p], prm=bad) == -1
    assert lib.nmod_fdr_adjust(None, 16, 1, None, 0, 0.05, None, None) == -1


def test_no_device_is_reported_and_empty_tracks_need_none():
    L, lib = _lib()
    p = np.full(4, 0.5)
    assert _call(lib, L, 4, [p]) == -5 and _call(lib, L, 4, [p], memspace=L.MEM_DEVICE) == -5
    assert b'no HIP device' in lib.nmod_strerror(-5)
    # n == 0: NMOD_OK, zero counts
    summ = (L.NmodFdrSummary * 2)()
    for s in summ:
        s.tested = s.excluded = s.rejected = 7
    parr = (C.c_void_p * 2)(p.ctypes.data, p.ctypes.data)
    prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST)
    assert lib.nmod_fdr_adjust(C.byref(prm), 0, 2, parr, 0, 0.05, parr, C.cast(summ, C.c_void_p)) == 0
    assert all((s.tested, s.excluded, s.rejected) == (0, 0, 0) and np.isnan(s.p_crit) for s in summ)


def test_python_layers_raise_the_library_error():
    import nanomod_amd as nm
    from nanomod_amd import detect, engine
    L = nm._lib
    p = np.linspace(0.0, 1.0, 32)
    with pytest.raises(L.NanomodLibraryError, match='nmod_fdr_adjust failed: no HIP device'):
        engine.fdr_adjust_host(p, device=NO_SUCH_DEVICE)
    with pytest.raises(L.NanomodLibraryError, match='nmod_fdr_adjust'):
        engine.fdr_adjust_host([p, p], method='by', alpha=0.01, device=NO_SUCH_DEVICE)
    with pytest.raises(L.NanomodLibraryError, match='invalid'):
        engine.fdr_adjust_host(p, alpha=2.0, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.fdr_adjust_host(p, method='storey', device=NO_SUCH_DEVICE)
    res = {'mwu_p': p, 't_p': p, 'ks_p': p, 'comb_p': p}
    with pytest.raises(L.NanomodLibraryError, match='nmod_fdr_adjust'):
        detect.fdr_tracks(res, True, 'bh', 0.05, NO_SUCH_DEVICE)
    with pytest.raises(KeyError):
        detect.fdr_tracks({'mwu_p': p, 't_p': p, 'ks_p': p}, True, 'bh', 0.05, NO_SUCH_DEVICE)
    with pytest.raises(ValueError, match='nmod_fdr'):
        detect._fdr_option({'nmod_fdr': 'storey'})
    assert detect._fdr_option({}) == '' and detect._fdr_option({'nmod_fdr': 'by'}) == 'by'
    assert callable(nm.DeviceDetector.fdr)


def test_cli_lists_the_flags_and_nmod_options_carries_them(capsys):
    from nanomod_amd import cli
    parser = cli.build_parser()
    with pytest.raises(SystemExit):
        parser.parse_args(['detect', '--help'])
    text = capsys.readouterr().out
    assert '--fdr {none,bh,by}' in text and '--fdrAlpha' in text
    base = ['detect', '--wrkBase1', 'a', '--wrkBase2', 'b']
    o = cli.nmod_options(parser.parse_args(base))
    assert o['nmod_fdr'] == '' and o['nmod_fdr_alpha'] == 0.05
    o = cli.nmod_options(parser.parse_args(base + ['--fdr', 'by', '--fdrAlpha', '0.01']))
    assert o['nmod_fdr'] == 'by' and o['nmod_fdr_alpha'] == 0.01
    assert cli.nmod_options(parser.parse_args(base + ['--fdr', 'none']))['nmod_fdr'] == ''
    with pytest.raises(SystemExit):
        parser.parse_args(base + ['--fdr', 'storey'])


def test_fdr_table_writer_format(tmp_path):
    from nanomod_amd import detect
    meta = dict(names=['chrA', 'chrB'], chrom_id=np.array([0, 1, 1], np.int32), strand=np.array(['+', '-', '+']),
                base=np.array(['A', 'C', 'G']), pos=np.array([9, 10, 11]))
    fdr = {'ks_q': np.array([0.5, np.nan, 1.0]), 'mwu_q': np.array([1e-12, 0.25, 0.0]), 't_q': np.array([np.nan, 0.125, 1.0]),
           'comb_q': np.array([3.25e-7, 1.0, np.nan])}
    path = tmp_path / 'x_sign_test_fdr.txt'
    detect.write_sign_test_fdr(str(path), meta, fdr)
    assert path.read_text() == ('chrA + 10 A 1.000E-12 NAN 5.000E-01 3.250E-07\n'
                                'chrB - 11 C 2.500E-01 1.250E-01 NAN 1.000E+00\n'
                                'chrB + 12 G 0.000E+00 1.000E+00 1.000E+00 NAN\n')
    del fdr['comb_q']
    detect.write_sign_test_fdr(str(path), meta, fdr)
    assert path.read_text().splitlines()[0] == 'chrA + 10 A 1.000E-12 NAN 5.000E-01'


def _mixed_track(rng, n):
    p = rng.random(n)
    p[rng.choice(n, n // 100, replace=False)] = rng.random(n // 100) * 1e-9            # planted small p-values
    sel = rng.choice(n, n // 3, replace=False)
    p[sel] = np.round(p[sel], 2)                                                       # ties
    p[rng.choice(n, 50, replace=False)] = 1.0
    p[rng.choice(n, 50, replace=False)] = np.finfo(np.float64).tiny
    p[rng.choice(n, 300, replace=False)] = np.nan
    return p


@pytest.mark.parametrize('method', ['bh', 'by'])
def test_restatement_equals_scipy(method):
    from scipy.stats import false_discovery_control
    rng = np.random.default_rng(20240917)
    p = _mixed_track(rng, 200000)
    ok = ~np.isnan(p)
    q = F.fdr_ref(p, method)
    assert np.array_equal(np.isnan(q), ~ok)
    assert np.array_equal(q[ok], false_discovery_control(p[ok], method=method))       # bit for bit
    assert np.array_equal(F.fdr_scipy(p, method), q, equal_nan=True)
    # the NaN rule: anything outside [0, 1] is left out like NaN
    p2 = p.copy(); bad = rng.choice(200000, 40, replace=False)
    p2[bad[:10]] = -1e-3; p2[bad[10:20]] = 1.0 + 2.0 ** -52; p2[bad[20:30]] = np.inf; p2[bad[30:]] = -np.inf
    ok2 = F.valid_mask(p2)
    assert not ok2[bad].any()
    assert np.array_equal(F.fdr_ref(p2, method)[ok2], false_discovery_control(p2[ok2], method=method))
    s = F.summary_ref(p2, F.fdr_ref(p2, method), 0.05)
    assert s['tested'] == ok2.sum() and s['excluded'] == 200000 - ok2.sum() and 0 < s['rejected'] < s['tested']
    assert s['p_crit'] == p2[ok2 & (F.fdr_ref(p2, method) <= 0.05)].max()
    # m <= 1: q = p
    assert np.array_equal(F.fdr_ref([np.nan, 0.25, 2.0], method), [np.nan, 0.25, np.nan], equal_nan=True)
    assert np.isnan(F.fdr_ref([np.nan], method)).all() and F.fdr_ref([], method).size == 0
