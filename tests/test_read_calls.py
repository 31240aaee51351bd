"""nmod_read_calls / nmod_site_calls (K12) without a GPU: the restatement pinned against mpmath, the declarations, the argument checks
(before any device work), the conditions the shared inputs must meet for the GPU gates, the two writers and the command line."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import readcalls_ref as Q
import rescale_ref as R
from nanomod_amd import readcalls as RC           # K12's module: without it nothing here can pass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def test_restatement_is_pinned_against_mpmath():
    """p, l and the window combination at |z| in {0, 1e-3, 1, 8, 30, 38, 40, 60} and W in {1, 5, 129} (and windows of zeros around one
    event beyond the clamp of p): within 1e-11 of mpmath where its value is above DBL_MIN, exactly DBL_MIN where it is below (asserted
    inside pin_agreement).  Measured: 6.3e-13 (p, l) and 1.2e-13 (windows); profiles/read_calls.txt."""
    worst_p, worst_w = Q.pin_agreement()
    print('restatement v mpmath: p / l %.3g, windows %.3g' % (worst_p, worst_w))
    assert worst_p <= Q.PIN_GATE and worst_w <= Q.PIN_GATE, (worst_p, worst_w)
    above = [float(Q.mp_window(zs)) >= Q.DBL_MIN for _, zs in Q.pin_windows()]
    assert sum(above) >= 12 and len(above) - sum(above) >= 12       # both sides of the clamp are pinned
    # p clamps from |z| = 37.52 on; the lone deep events of the deep-tail read sit beyond it, their windows do not
    assert Q.tails(np.array([37.0]))[0][0] > Q.DBL_MIN and Q.tails(np.array([37.6]))[0][0] == Q.DBL_MIN
    (_, z38), (_, z39) = Q.DEEP_SINGLES
    lone = lambda h, z: float(Q.mp_window([0.0] * h + [z] + [0.0] * h))
    assert float(Q.mp_tails(z38)[0]) < Q.DBL_MIN and float(Q.mp_tails(z39)[0]) < Q.DBL_MIN
    assert lone(2, z38) > Q.DBL_MIN and lone(64, z38) > Q.DBL_MIN and lone(64, z39) > Q.DBL_MIN > lone(2, z39)


def test_restatement_windows_by_hand():
    """a read of 6 events over a 1-mer model, two of them ineligible: W counts the events that exist, the ends have shorter windows, and
    nb = 0 hands p through"""
    mean, sd = np.array([0.0, np.nan, 0.0, 0.0]), np.array([1.0, 1.0, 2.0, 1.0])
    base = np.frombuffer(b'ACGNTA', np.uint8)
    x = np.array([1.0, 5.0, -3.0, 0.5, np.inf, 2.0])
    codes = R.read_codes(base, 1, 0)
    z, p, P, W = Q.score_read(x, codes, mean, sd, 1)
    assert codes.tolist() == [0, 1, 2, -1, 3, 0] and W.tolist() == [1, 0, 1, 0, 0, 1]
    assert np.array_equal(z[[0, 2, 5]], [1.0, -1.5, 2.0]) and np.isnan(z[[1, 3, 4]]).all() and np.isnan(P[[1, 3, 4]]).all()
    z, p, P, W = Q.score_read(x, codes, mean, sd, 2)
    assert W.tolist() == [2, 0, 2, 0, 0, 1]                       # events 0 and 2 see each other; event 5 sees nobody
    import mpmath as mp
    for j, zs in ((0, [1.0, -1.5]), (2, [1.0, -1.5]), (5, [2.0])):
        assert abs(P[j] / float(Q.mp_window(zs)) - 1.0) <= 1e-13
    z0, p0, P0, W0 = Q.score_read(x, codes, mean, sd, 0)
    assert P0.tobytes() == p0.tobytes() and abs(p0[0] / float(mp.erfc(mp.mpf(1.0) / mp.sqrt(2))) - 1.0) <= 1e-15
    s = Q.site_calls(np.array([0.01, 0.5, np.nan, 1.5, -0.1, 0.0, 1.0]), np.array([0, 3, 3, 5, 7]), 0.01)
    assert s['n_valid'].tolist() == [2, 0, 0, 2] and s['n_called'].tolist() == [1, 0, 0, 1]
    assert s['frac'][[0, 3]].tolist() == [0.5, 0.5] and np.isnan(s['frac'][[1, 2]]).all()


def test_entries_are_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    declared = set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    for name in ('nmod_read_calls', 'nmod_site_calls'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name)
    assert '#define NMOD_CALLS_TOO_LARGE 16' in header and L.CALLS_TOO_LARGE == Q.TOO_LARGE == 16
    assert '#define NMOD_CALLS_WAVE_MAX 2048' in header and L.CALLS_WAVE_MAX == Q.WAVE_MAX == 2048
    assert L.MAX_NB == Q.MAX_NB == 64 and L.MAX_DEEP == Q.MAX_DEEP
    assert 'typedef struct nmod_calls_opts { int32_t struct_size, nb; double alpha; } nmod_calls_opts;' in header
    assert re.search(r'typedef struct nmod_calls_out \{ int32_t struct_size; int32_t reserved;\s+double \*z, \*p, \*p_win;[^\n]*\n\s+'
                     r'int32_t \*n_sites, \*n_called; uint8_t\* status;', header)
    assert 'typedef struct nmod_site_out { int32_t struct_size; int32_t reserved; int32_t *n_valid, *n_called; double* frac; } nmod_site_out;' in header
    assert C.sizeof(L.NmodCallsOpts) == 16 and C.sizeof(L.NmodCallsOut) == 56 and C.sizeof(L.NmodSiteOut) == 32
    assert L.NmodCallsOpts.alpha.offset == 8 and L.NmodCallsOut.z.offset == 8 and L.NmodCallsOut.status.offset == 48
    assert L.NmodSiteOut.n_valid.offset == 8 and L.NmodSiteOut.frac.offset == 24
    assert [n for n, _ in L.NmodCallsOut._fields_[2:]] == ['z', 'p', 'p_win', 'n_sites', 'n_called', 'status']
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # purely additive entries
    assert 0.70710678118654752 == Q.INV_SQRT2 and 'u_j = |z_j| * 0.70710678118654752' in header


def _call(lib, L, nreads=3, *, off='x', val='x', base='x', model='x', k=3, center=1, mean='x', sd='x', opts='x', out='x', nb=2, alpha=0.01,
          dtype=None, memspace=None, prm=None, opts_size=None, out_size=None, z='x'):
    n = nreads if 0 <= nreads < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 60
    x, b = np.zeros(max(n, 1) * 60, np.int16), np.full(max(n, 1) * 60, ord('A'), np.uint8)
    mu, s = np.zeros(4 ** 8), np.ones(4 ** 8)
    ev = np.zeros(max(n, 1) * 60)
    cnt = np.zeros(max(n, 1), np.int32)
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    m = L.NmodRescaleModel()
    m.k, m.center, m.mean, m.sd = k, center, pick(mean, mu), pick(sd, s)
    o = L.make_calls_opts(nb, alpha)
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_calls_out(z=pick(z, ev), n_sites=cnt.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_I16_MILLI if dtype is None else dtype)
    return lib.nmod_read_calls(C.byref(prm), nreads, pick(off, offs), pick(val, x), pick(base, b), C.byref(m) if model is not None else None,
                               C.byref(o) if opts is not None else None, C.byref(r) if out is not None else None)


def test_read_calls_refuses_invalid_arguments_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    nan, inf = float('nan'), float('inf')
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5 and _call(lib, L, dtype=L.DTYPE_F32) == -5 and _call(lib, L, dtype=L.DTYPE_F64) == -5
    assert _call(lib, L, nb=0) == -5 and _call(lib, L, nb=64) == -5 and _call(lib, L, alpha=1.0) == -5 and _call(lib, L, alpha=1e-300) == -5
    assert _call(lib, L, k=1, center=0) == -5 and _call(lib, L, k=8, center=7) == -5 and _call(lib, L, z=None) == -5
    assert _call(lib, L, 0) == 0 and _call(lib, L, 0, off=None, val=None, base=None, mean=None, sd=None) == 0     # no reads: no device needed
    assert _call(lib, L, nb=-1) == -1 and _call(lib, L, nb=65) == -1
    assert all(_call(lib, L, alpha=v) == -1 for v in (0.0, -0.01, 1.0000001, nan, inf, -inf))
    assert _call(lib, L, k=0, center=0) == -1 and _call(lib, L, k=9) == -1 and _call(lib, L, center=3) == -1 and _call(lib, L, center=-1) == -1
    assert _call(lib, L, off=None) == -1 and _call(lib, L, val=None) == -1 and _call(lib, L, base=None) == -1
    assert _call(lib, L, model=None) == -1 and _call(lib, L, mean=None) == -1 and _call(lib, L, sd=None) == -1
    assert _call(lib, L, opts_size=8) == -1 and _call(lib, L, opts_size=24) == -1 and _call(lib, L, opts=None) == -1
    assert _call(lib, L, out_size=48) == -1 and _call(lib, L, out_size=64) == -1 and _call(lib, L, out=None) == -1
    assert _call(lib, L, dtype=3) == -1 and _call(lib, L, dtype=-1) == -1 and _call(lib, L, memspace=2) == -1
    assert _call(lib, L, -1) == -1 and _call(lib, L, 2 ** 32 - 1) == -1 and _call(lib, L, 2 ** 40) == -1
    assert _call(lib, L, off=np.array([0, 60, 40, 180], np.int64)) == -1        # host offsets that decrease
    assert _call(lib, L, off=np.array([-1, 60, 120, 180], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, prm=bad) == -1
    assert lib.nmod_read_calls(None, 3, None, None, None, None, None, None) == -1


def _site(lib, L, npos=3, *, score='x', off='x', stride=0, alpha=0.01, out='x', out_size=None, memspace=None, prm=None, dtype=7):
    n = npos if 0 <= npos < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 5
    sc = np.zeros(max(n, 1) * 5)
    cnt, fr = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    r = L.make_site_out(n_valid=cnt.ctypes.data, frac=fr.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:                                                             # (dtype 7: this entry does not read it)
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace, dtype=dtype, stride0=stride)
    return lib.nmod_site_calls(C.byref(prm), npos, pick(score, sc), pick(off, offs), alpha, C.byref(r) if out is not None else None)


def test_site_calls_refuses_invalid_arguments_before_any_device_work():
    L, lib = _lib()
    nan, inf = float('nan'), float('inf')
    assert _site(lib, L) == -5 and _site(lib, L, off=None, stride=5) == -5 and _site(lib, L, memspace=L.MEM_DEVICE) == -5
    assert _site(lib, L, alpha=1.0) == -5 and _site(lib, L, dtype=L.DTYPE_F32) == -5
    assert _site(lib, L, 0) == 0 and _site(lib, L, 0, score=None) == 0
    assert all(_site(lib, L, alpha=v) == -1 for v in (0.0, -1.0, 1.5, nan, inf))
    assert _site(lib, L, off=None) == -1 and _site(lib, L, off=None, stride=-5) == -1          # neither offsets nor a stride
    assert _site(lib, L, -1) == -1 and _site(lib, L, 2 ** 31 - 1) == -1 and _site(lib, L, 2 ** 40) == -1
    assert _site(lib, L, score=None) == -1 and _site(lib, L, out=None) == -1 and _site(lib, L, out_size=24) == -1 and _site(lib, L, memspace=2) == -1
    assert _site(lib, L, off=np.array([0, 5, 4, 15], np.int64)) == -1 and _site(lib, L, off=np.array([-1, 5, 10, 15], np.int64)) == -1
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _site(lib, L, prm=bad) == -1
    assert lib.nmod_site_calls(None, 3, None, None, 0.01, None) == -1


def test_python_layers_raise_for_the_same_inputs():
    import nanomod_amd
    from nanomod_amd import engine
    mean, sd = R.make_model(3)
    model = dict(k=3, center=1, mean=mean, sd=sd)
    val, off, base = np.zeros(120, np.int16), np.array([0, 60, 120], np.int64), np.full(120, b'A', 'S1')
    call = lambda **kw: engine.read_calls_host(kw.pop('val', val), kw.pop('off', off), kw.pop('base', base), kw.pop('model', model),
                                               device=NO_SUCH_DEVICE, **kw)
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_read_calls'):
        call()                                                                  # well-formed: only the device is missing
    for kw in (dict(nb=-1), dict(nb=65), dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float('nan')), dict(model=dict(model, k=0)),
               dict(model=dict(model, k=9)), dict(model=dict(model, center=3)), dict(model=None), dict(want=('q',)),
               dict(val=val.astype(np.int32)), dict(off=np.array([0, 70, 60], np.int64)), dict(off=np.array([0, 60, 121], np.int64)),
               dict(base=base[:100]), dict(model=dict(model, mean=mean[:10]))):
        with pytest.raises(ValueError):
            call(**kw)
    res = call(val=val[:0], off=np.zeros(1, np.int64), base=base[:0], want=('p_win',))          # no reads: no device needed
    assert res['p_win'].shape == (0,) and res['n_called'].shape == (0,) and 'z' not in res
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_site_calls'):
        engine.site_calls_host(np.zeros(10), np.array([0, 4, 10], np.int64), device=NO_SUCH_DEVICE)
    for args, kw in (((np.zeros(10), np.array([0, 4, 10], np.int64)), dict(alpha=0.0)), ((np.zeros(10), None), dict()),
                     ((np.zeros(10), None), dict(stride=3)), ((np.zeros(10), np.array([0, 4, 11], np.int64)), dict()),
                     ((np.zeros(10), np.array([0, 6, 4], np.int64)), dict())):
        with pytest.raises(ValueError):
            engine.site_calls_host(*args, device=NO_SUCH_DEVICE, **kw)
    assert engine.site_calls_host(np.zeros(0), np.zeros(1, np.int64))['frac'].shape == (0,)
    reads = dict(chrom=['c'] * 2, strand=['+'] * 2, start=[0, 0], off=off, norm_mean=val, base=base)
    with pytest.raises(ValueError, match='unknown option'):
        RC.call_reads(reads, dict(model, n_positions=np.ones(64, np.int64)), rescale=dict(drop_failed=True), device=NO_SUCH_DEVICE)
    assert nanomod_amd.call_reads is RC.call_reads and nanomod_amd.read_calls_host is engine.read_calls_host
    assert nanomod_amd.site_calls_host is engine.site_calls_host and nanomod_amd.write_site_calls is RC.write_site_calls


@pytest.mark.parametrize('k,center', Q.PARITY_KC)
@pytest.mark.parametrize('nb', Q.PARITY_NB)
def test_parity_inputs_meet_the_conditions_of_the_gpu_gates(k, center, nb):
    """the restatement has no window p-value within 1e-9 (relative) of alpha — so n_called is an exact integer to compare — and the
    inputs reach both sides of the clamp, ineligible events of every kind, and both size classes"""
    for dtype in Q.PARITY_DTYPES:
        p = Q.parity_inputs(k, center, nb, dtype)
        exp = Q.parity_expected(k, center, nb, dtype)
        lens = np.diff(p['off'])
        assert lens.tolist() == Q.parity_lengths(k, nb) and lens.max() == 70000 and (lens == Q.WAVE_MAX + 1).any()
        assert exp['alpha_margin'] > 1e-9
        P = exp['p_win']
        assert np.isnan(P).sum() >= 4 and (P == Q.DBL_MIN).sum() >= 4 and ((P > Q.DBL_MIN) & (P < 1e-3)).sum() >= 100
        assert (exp['n_called'] > 0).sum() >= 6 and (exp['n_sites'][lens >= 63] > 0).all() and not exp['status'].any()
        if nb:
            assert exp['W'].max() == 2 * nb + 1 and ((exp['W'] > 0) & (exp['W'] < nb + 1)).any()      # full windows, and holes inside windows


def test_chain_inputs_carry_the_planted_position():
    """the planted position has the largest n_called of its strand in the restatement: the precondition of the GPU chain test.  Without
    a window (nb = 0) the shift of one event is one position's; with nb = 2 every window that holds the shifted event carries it, so the
    five positions around it share the calls and the largest count lies within 2 of the planted position."""
    reads, model, planted = Q.chain_inputs()
    n = np.diff(reads['off'])
    assert len(n) == 200 and n.min() >= 300 and n.max() <= 600 and set(reads['strand']) == {'+', '-'}
    for nb in Q.CHAIN_NB:
        exp = Q.read_calls(reads['norm_mean'], reads['off'], reads['base'], 3, 1, model['mean'], model['sd'], nb, 0.01)
        assert exp['alpha_margin'] > 1e-9
        rows = Q.pivot(reads, exp['p_win'])
        s = Q.site_calls(rows['val'], rows['off'], 0.01)
        for strand in '+-':
            m = rows['strand'] == strand
            best = np.flatnonzero(m)[np.argmax(s['n_called'][m])]
            at = np.flatnonzero(m & (rows['pos'] == planted))[0]
            assert np.diff(rows['off'])[at] == 100                                                 # every read of the strand covers it
            assert abs(rows['pos'][best] - planted) <= nb and s['n_called'][best] >= 30, (nb, strand, rows['pos'][best], s['n_called'][best])
            if nb == 0:                                                                            # ~0.92 of the 50 shifted reads, ~1 of the others
                others = s['n_called'][m & (rows['pos'] != planted)]
                assert s['n_called'][at] >= 40 and others.max() <= 8, (strand, s['n_called'][at], others.max())


def test_writers():
    table = dict(index=np.arange(3), chrom=np.array(['chr1', 'chr2', 'chr2']), strand=np.array(['+', '-', '+']), start=np.array([5, 70, 9], np.int64),
                 events=np.array([200, 1, 300]), n_sites=np.array([198, 0, 297], np.int32), n_called=np.array([4, 0, 31], np.int32),
                 status=np.array([0, 0, 16], np.uint8))
    sites = dict(chrom=np.array(['chr1', 'chr1', 'chr2']), strand=np.array(['+', '-', '+']), pos=np.array([0, 41, 7], np.int64),
                 base=np.array(['A', 'c', 'N']), n_reads=np.array([3, 2, 1], np.int32), n_valid=np.array([3, 0, 1], np.int32),
                 n_called=np.array([1, 0, 1], np.int32), frac=np.array([1.0 / 3.0, np.nan, 1.0]))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 't.txt')
        RC.write_read_calls(path, table)
        assert open(path).read() == '0 chr1 + 5 200 198 4 0\n1 chr2 - 70 1 0 0 0\n2 chr2 + 9 300 297 31 16\n'
        RC.write_site_calls(path, sites)
        assert open(path).read() == 'chr1 + 1 A 3 3 1 0.333333\nchr1 - 42 c 2 0 0 nan\nchr2 + 8 N 1 1 1 1.000000\n'


def test_cli_parser_and_checks(capsys):
    from nanomod_amd import cli, container
    p = cli.build_parser()
    a = p.parse_args(['readcalls', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz'])
    assert (a.cmd, a.wrkBase1, a.kmerModel, a.neighborPvalues, a.callAlpha, a.minPositions, a.rescale, a.outEvents, a.outFolder, a.FileID, a.device,
            a.outLevel) == ('readcalls', 'r.npz', 'm.npz', 2, 0.01, 1, 0, '', 'mRes', 'mod', 0, 2)
    a = p.parse_args(['readcalls', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--neighborPvalues', '5', '--callAlpha', '0.001', '--minPositions', '3',
                      '--rescale', '1', '--outEvents', 'e.npz', '--outFolder', 'd', '--FileID', 'id', '--device', '1', '--outLevel', '3'])
    assert (a.neighborPvalues, a.callAlpha, a.minPositions, a.rescale, a.outEvents, a.outFolder, a.FileID, a.device, a.outLevel) == \
        (5, 0.001, 3, 1, 'e.npz', 'd', 'id', 1, 3)
    for argv in (['readcalls'], ['readcalls', '--wrkBase1', 'r.npz'], ['readcalls', '--kmerModel', 'm.npz'],
                 ['readcalls', '--wrkBase1', 'r.npz', '--kmerModel', 'm.npz', '--rescale', '2']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    capsys.readouterr()
    assert cli.main(['readcalls', '--wrkBase1', '/nonexistent/r.npz', '--kmerModel', '/nonexistent/m.npz']) == 1
    out = capsys.readouterr().out
    assert 'Error: input /nonexistent/r.npz does not exist' in out and 'Error: input /nonexistent/m.npz does not exist' in out
    with tempfile.TemporaryDirectory() as tmp:
        reads, group, other = (os.path.join(tmp, n) for n in ('r.npz', 'g.npz', 'm.npz'))
        container.save_reads(reads, ['c'], ['+'], [0], [0, 2], np.array([0.5, 0.25]), np.array([b'A', b'C']))
        container.save_group(group, ['c'], ['+'], [0], ['A'], [0, 1], np.zeros(1, np.float32))
        np.savez(other, x=np.zeros(1))
        base = ['readcalls', '--kmerModel', other]
        assert cli.main(base + ['--wrkBase1', group]) == 1                      # a per-position container has no reads
        assert 'Error: --wrkBase1 %s is not a read-level container (per-position containers have no reads)' % group in capsys.readouterr().out
        for bad, msg in ((['--neighborPvalues', '65'], 'Error: --neighborPvalues should be in 0 .. 64'),
                         (['--neighborPvalues', '-1'], 'Error: --neighborPvalues should be in 0 .. 64'),
                         (['--callAlpha', '0'], 'Error: --callAlpha should be larger than 0 and not larger than 1'),
                         (['--callAlpha', '1.5'], 'Error: --callAlpha should be larger than 0 and not larger than 1'),
                         (['--minPositions', '0'], 'Error: --minPositions should be larger than 0')):
            assert cli.main(base + ['--wrkBase1', reads] + bad) == 1
            assert msg in capsys.readouterr().out
