"""nmod_kmer_mix (K17) without a GPU: the declaration, the argument checks (before any device work), the restatement
(tests/kmix_ref.py) against 40-digit mpmath, the recovery conditions on the restatement, and the pure parts of
kmermodel.learn_alt_model: the selection rule, the model container and the table writer."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

import kmix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def test_kmer_mix_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_kmer_mix' in set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    assert 'nmod_kmer_mix' in L._SIGNATURES and hasattr(lib, 'nmod_kmer_mix')
    for name, lv, rv in (('HALF', L.KMIX_HALF, R.HALF), ('BINS', L.KMIX_BINS, R.BINS), ('NOT_CONVERGED', L.KMIX_NOT_CONVERGED, R.NOT_CONVERGED),
                         ('DEGENERATE', L.KMIX_DEGENERATE, R.DEGENERATE), ('NO_MODEL', L.KMIX_NO_MODEL, R.NO_MODEL),
                         ('VAR_FLOORED', L.KMIX_VAR_FLOORED, R.VAR_FLOORED), ('TOO_FEW', L.KMIX_TOO_FEW, R.TOO_FEW)):
        m = re.search(r'#define NMOD_KMIX_%s\s+(\d+)' % name, header)
        assert m and int(m.group(1)) == lv == rv, name
    assert (L.STATUS_EMPTY, L.STATUS_TOO_LARGE, L.STATUS_NONFINITE, L.STATUS_NO_CODE, L.MAX_DEEP) == \
           (R.ST_EMPTY, R.ST_TOO_LARGE, R.ST_NONFINITE, R.ST_NO_CODE, R.MAX_DEEP)
    assert (L.MIX_EQUAL_VAR, L.MIX_FREE_VAR) == (R.EQUAL, R.FREE)
    assert C.sizeof(L.NmodKmixOpts) == 32 and L.NmodKmixOpts.min_samples.offset == 16 and L.NmodKmixOpts.tol.offset == 24
    assert C.sizeof(L.NmodKmixOut) == 96 and L.NmodKmixOut.n_positions.offset == 8 and L.NmodKmixOut.pos_status.offset == 88
    assert [n for n, _ in L.NmodKmixOut._fields_][2:] == ['n_positions', 'n_used', 'n_outside', 'pi', 'mu_mod', 'sd_mod', 'llr', 'iters',
                                                          'status', 'hist', 'pos_status']
    assert lib.nmod_kmer_mix.argtypes == L._SIGNATURES['nmod_kmer_mix'][1] and len(lib.nmod_kmer_mix.argtypes) == 10
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # a purely additive entry


def _call(lib, L, npos=4, *, sig='x', off='x', code='x', ncodes=16, mean0='x', sd0='x', opts='x', out='x', dtype=None, stride=0, memspace=None,
          prm=None, struct_size=None, res=None, **o):
    n = max(npos, 1) if 0 <= npos < 1000 else 4
    x = np.zeros(n * 8, np.int16)
    offs = np.arange(n + 1, dtype=np.int64) * 8
    codes = np.arange(n, dtype=np.int32) % 4
    m = ncodes if 1 <= ncodes <= 65536 else 1
    mu, sd = np.zeros(m), np.full(m, 0.2)
    if res is None:
        res = dict({k: np.zeros(m, np.int64) for k in L.KMIX_COUNT_FIELDS}, **{k: np.zeros(m) for k in L.KMIX_FIELDS})
        res.update(iters=np.zeros(m, np.int32), status=np.zeros(m, np.uint8), pos_status=np.zeros(n, np.uint8))
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    ko = L.make_kmix_out(**{k: a.ctypes.data for k, a in res.items()})
    if struct_size is not None:
        ko.struct_size = struct_size
    op = L.make_kmix_opts()
    for k, v in o.items():
        setattr(op, k, v)
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_I16_MILLI if dtype is None else dtype, stride0=stride)
    return lib.nmod_kmer_mix(C.byref(prm), npos, pick(sig, x), pick(off, offs), pick(code, codes), ncodes, pick(mean0, mu), pick(sd0, sd),
                             C.byref(op) if opts is not None else None, C.byref(ko) if out is not None else None)


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5 and _call(lib, L, off=None, stride=8) == -5
    assert _call(lib, L, dtype=L.DTYPE_F32) == -5 and _call(lib, L, dtype=L.DTYPE_F64) == -5
    assert _call(lib, L, model=0) == -5 and _call(lib, L, max_iter=1) == -5 and _call(lib, L, max_iter=10000) == -5
    assert _call(lib, L, tol=0.0) == -5 and _call(lib, L, min_samples=0) == -5
    assert _call(lib, L, code=np.array([-1, 15, 0, -1], np.int32)) == -5 and _call(lib, L, ncodes=65536) == -5
    assert _call(lib, L, -1) == -1 and _call(lib, L, 2 ** 31 - 1) == -1 and _call(lib, L, 2 ** 40) == -1
    assert _call(lib, L, ncodes=0) == -1 and _call(lib, L, ncodes=65537) == -1 and _call(lib, L, ncodes=-4) == -1
    assert _call(lib, L, mean0=None) == -1 and _call(lib, L, sd0=None) == -1 and _call(lib, L, opts=None) == -1 and _call(lib, L, out=None) == -1
    assert _call(lib, L, model=2) == -1 and _call(lib, L, model=-1) == -1
    assert _call(lib, L, max_iter=0) == -1 and _call(lib, L, max_iter=10001) == -1
    assert _call(lib, L, tol=-1e-9) == -1 and _call(lib, L, tol=float('nan')) == -1 and _call(lib, L, tol=float('inf')) == -1
    assert _call(lib, L, min_samples=-1) == -1
    assert _call(lib, L, struct_size=88) == -1 and _call(lib, L, struct_size=104) == -1          # the out struct
    assert _call(lib, L, **{'struct_size': 96}) == -5
    bad = L.make_kmix_opts(); bad.struct_size = 24                                            # the opts struct
    prm = L.make_params(device=NO_SUCH_DEVICE, dtype=L.DTYPE_I16_MILLI, stride0=8)
    z = np.zeros(64, np.int16); cz = np.zeros(4, np.int32); mu = np.zeros(16); sd = np.ones(16)
    ko = L.make_kmix_out()
    args = (C.byref(prm), 4, z.ctypes.data, None, cz.ctypes.data, 16, mu.ctypes.data, sd.ctypes.data)
    assert lib.nmod_kmer_mix(*args, C.byref(bad), C.byref(ko)) == -1
    assert lib.nmod_kmer_mix(*args, C.byref(L.make_kmix_opts()), C.byref(ko)) == -5
    assert _call(lib, L, sig=None) == -1 and _call(lib, L, code=None) == -1
    assert _call(lib, L, off=None) == -1                                        # neither offsets nor a stride
    assert _call(lib, L, dtype=3) == -1 and _call(lib, L, dtype=-1) == -1
    assert _call(lib, L, off=np.array([0, 8, 4, 12, 16], np.int64)) == -1       # host offsets that decrease
    assert _call(lib, L, code=np.array([0, 16, 0, 0], np.int32)) == -1          # host memory: a code outside [-1, ncodes)
    assert _call(lib, L, code=np.array([0, -2, 0, 0], np.int32)) == -1
    assert _call(lib, L, code=np.array([0, 16, 0, 0], np.int32), memspace=L.MEM_DEVICE) == -5     # (device memory: NO_CODE per position)
    badp = L.make_params(device=NO_SUCH_DEVICE); badp.struct_size -= 4
    assert _call(lib, L, prm=badp) == -1
    assert lib.nmod_kmer_mix(None, 4, None, None, None, 16, None, None, None, None) == -1


def test_no_positions_is_ok_with_zero_counts_and_too_few():
    L, lib = _lib()
    res = dict({k: np.full(16, 7, np.int64) for k in L.KMIX_COUNT_FIELDS}, **{k: np.zeros(16) for k in L.KMIX_FIELDS})
    res.update(iters=np.full(16, 5, np.int32), status=np.zeros(16, np.uint8), hist=np.full(16 * L.KMIX_BINS, 3, np.uint32))
    mu = np.zeros(16); mu[3] = np.nan; mu[4] = 2000.0
    sd = np.full(16, 0.2); sd[5] = 0.0; sd[6] = np.inf
    assert _call(lib, L, 0, res=res, mean0=mu, sd0=sd) == 0
    assert all(not res[k].any() for k in L.KMIX_COUNT_FIELDS) and all(np.isnan(res[k]).all() for k in L.KMIX_FIELDS)
    assert not res['iters'].any() and not res['hist'].any()
    want = np.full(16, L.KMIX_TOO_FEW, np.uint8); want[3:7] = L.KMIX_NO_MODEL
    assert np.array_equal(res['status'], want)
    assert _call(lib, L, 0, sig=None, off=None, code=None) == 0


def test_python_layers_report_the_missing_device_and_bad_arguments():
    import nanomod_amd
    from nanomod_amd import engine
    x, off, code = np.zeros(8, np.int16), np.array([0, 4, 8], np.int64), np.zeros(2, np.int32)
    mu, sd = np.zeros(4), np.ones(4)
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_kmer_mix'):
        engine.kmer_mix_host(x, off, code, 4, mu, sd, device=NO_SUCH_DEVICE)
    for kw in (dict(model='both'), dict(model=2), dict(max_iter=0), dict(max_iter=10001), dict(tol=-1.0), dict(tol=float('nan')),
               dict(min_samples=-1), dict(min_samples=2.5)):
        with pytest.raises(ValueError):
            engine.kmer_mix_host(x, off, code, 4, mu, sd, device=NO_SUCH_DEVICE, **kw)
    with pytest.raises(ValueError):
        engine.kmer_mix_host(x, off, code, 4, np.zeros(3), sd, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_mix_host(x, off, code, 4, mu, None, device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.kmer_mix_host(x.astype(np.int32), off, code, 4, mu, sd, device=NO_SUCH_DEVICE)


# ------------------------------------------------------------------------------------------------------- the restatement
def test_restated_histogram_on_a_hand_made_batch():
    mean0 = np.array([0.0, 1.0, np.nan, 2000.0])
    sd0 = np.array([0.2, 0.2, 0.2, 0.2])
    lo = R.window_lo(mean0)
    assert lo[0] == -2048 and lo[1] == -1048 and list(R.usable(mean0, sd0)) == [True, True, False, False]
    rows = [[-2049, -2048, 2047, 2048], [], [5, 5, 5], [1, 2], [7], [9], [3000]]
    code = [0, 0, 1, 2, -1, 3, 0]
    sig, off = R.csr(rows)
    h = R.hist(sig, off, code, 4, mean0, sd0)
    assert list(h['n_used']) == [2, 3, 0, 0] and list(h['n_outside']) == [3, 0, 0, 0] and list(h['n_positions']) == [1, 1, 0, 0]
    assert h['hist'][0][0] == 1 and h['hist'][0][4095] == 1 and h['hist'][1][5 + 1048] == 3 and h['hist'].sum() == 5
    assert list(h['pos_status']) == [0, R.ST_EMPTY, 0, 0, R.ST_NO_CODE, 0, 0]
    f = R.hist(np.array([0.0005, 0.0015, 0.0025, np.nan, np.inf, 1e306]), np.array([0, 6]), [0], 1, mean0[:1], sd0[:1])
    assert f['hist'][0][2048] == 1 and f['hist'][0][2050] == 2 and f['n_used'][0] == 3          # ties to even: 0, 2, 2
    assert f['n_outside'][0] == 3 and f['pos_status'][0] == R.ST_NONFINITE


def _planted_hist(rng, n, share, shift_sd, mean0=0.37, sd0=0.21):
    y = mean0 + sd0 * rng.standard_normal(n)
    y[rng.random(n) < share] += shift_sd * sd0
    k = np.rint(1000.0 * y).astype(np.int64)
    lo = int(R.window_lo(np.array([mean0]))[0])
    return np.bincount(k - lo, minlength=R.BINS)[:R.BINS], lo, mean0, sd0


@pytest.mark.parametrize('model', [R.EQUAL, R.FREE])
def test_the_restatement_agrees_with_mpmath_at_30_iterations(model):
    """pi, m / s, sqrt v and llr of the double-precision restatement against 40 digits: 1e-12 relative.  The 1e-9 of the GPU parity
    test hides no conditioning."""
    pytest.importorskip('mpmath')
    rng = np.random.default_rng(20261022)
    for n, share, shift in ((40, 0.5, 4.0), (300, 0.3, 3.0), (300, 0.0, 3.0), (2000, 0.1, -5.0), (2000, 1.0, 3.0), (5000, 0.6, 4.0)):
        h, lo, mu, sd = _planted_hist(rng, n, share, shift)
        o, q = R.em(h, lo, mu, sd, model, 30), R.em_mp(h, lo, mu, sd, model, 30)
        assert o['status'] & ~R.VAR_FLOORED == 0
        tag = (n, share, shift, model)
        assert abs(o['pi'] - q['pi']) <= 1e-12 * q['pi'], tag
        assert abs(o['mu_mod'] - q['mu_mod']) <= 1e-12 * max(abs(q['mu_mod']), sd), tag
        assert abs(o['sd_mod'] - q['sd_mod']) <= 1e-12 * q['sd_mod'], tag
        assert abs(o['llr'] - q['llr']) <= 1e-12 * abs(q['llr']) + 1e-12 * n, tag


def test_restated_status_words():
    rng = np.random.default_rng(5)
    h, lo, mu, sd = _planted_hist(rng, 500, 0.4, 4.0)
    assert R.run(h, lo, np.nan, sd, R.FREE)['status'] == R.NO_MODEL and R.run(h, lo, mu, 0.0, R.FREE)['status'] == R.NO_MODEL
    assert R.run(h, lo, 1000.5, sd, R.FREE)['status'] == R.NO_MODEL
    assert R.run(h, lo, mu, sd, R.FREE, min_samples=501)['status'] == R.TOO_FEW and R.run(h, lo, mu, sd, R.FREE, min_samples=500)['iters'] > 0
    one = np.zeros(R.BINS, np.int64); one[100] = 1
    assert R.run(one, lo, mu, sd, R.FREE, min_samples=0)['status'] == R.TOO_FEW           # below 2 whatever min_samples says
    a = R.run(h, lo, mu, sd, R.FREE, max_iter=3)
    assert a['status'] & R.NOT_CONVERGED and a['iters'] == 3
    b = R.run(h, lo, mu, sd, R.FREE, max_iter=10000, tol=1e-6)
    assert not b['status'] & R.NOT_CONVERGED and b['delta'] <= 1e-6 < b['delta_prev']
    assert abs(b['pi'] - 0.4) < 0.1 and abs(b['mu_mod'] - (mu + 4.0 * sd)) < 0.5 * sd
    z = R.run(h, lo, mu, sd, R.FREE, max_iter=7, tol=0.0)
    assert z['iters'] == 7 and z['status'] & R.NOT_CONVERGED
    two = np.zeros(R.BINS, np.int64); two[3900] = 40; two[3901] = 60                       # far from mean0, two adjacent bins: the floor
    fl = R.run(two, lo, mu, sd, R.FREE)
    assert fl['status'] & R.VAR_FLOORED and fl['sd_mod'] == pytest.approx(sd / 4.0, rel=1e-15) and fl['pi'] > 0.999


# ------------------------------------------------------------------------------------------ recovery, on the restatement
def _table_from(group, k, center):
    """the control's k-mer table as build_kmer_model defines it (K10: the pooled mean and ddof-0 sd per code), in numpy"""
    from nanomod_amd import kmermodel
    code = kmermodel.group_codes(group, k, center)
    x = group['sig'].astype(np.float64).reshape(len(code), -1) / 1000.0
    mean0, sd0 = np.full(4 ** k, np.nan), np.full(4 ** k, np.nan)
    for c in np.unique(code[code >= 0]):
        v = x[code == c].reshape(-1)
        mean0[c], sd0[c] = v.mean(), v.std()
    return code, mean0, sd0


def test_recovery_conditions_hold_for_the_restatement():
    """The bounds the GPU recovery test asserts through learn_alt_model are conditions on the definition: with min_samples 1 000,
    min_pi 0.05, min_shift 1.0 exactly the two planted 3-mers are kept, |pi - 0.5| <= 0.05 and |mu_mod - (mean0 + 0.8)| <= 0.25 sd0."""
    from nanomod_amd import kmermodel
    cfg = R.RECOVERY
    control, sample, planted = R.recovery_groups()
    _, mean0, sd0 = _table_from(control, cfg['k'], cfg['center'])
    code = kmermodel.group_codes(sample, cfg['k'], cfg['center'])
    res = R.restated_alt(sample, code, mean0, sd0)
    kept = kmermodel.select_alt_codes(res, mean0, sd0, 1000, 0.05, 1.0)
    shift = np.abs(res['mu_mod'] - mean0) / sd0
    null = np.setdiff1d(np.flatnonzero(res['n_used'] >= 1000), planted)
    print('kept', np.flatnonzero(kept), 'planted', planted, 'n_used', res['n_used'][planted], 'pi', res['pi'][planted],
          'level error / sd0', (res['mu_mod'][planted] - mean0[planted] - cfg['shift']) / sd0[planted])
    print('null codes with pi >= 0.05: largest shift / sd0 %.3f' % np.nanmax(np.where(res['pi'][null] >= 0.05, shift[null], 0.0)))
    assert np.array_equal(np.flatnonzero(kept), planted)
    assert np.all(np.abs(res['pi'][planted] - cfg['share']) <= 0.05)
    assert np.all(np.abs(res['mu_mod'][planted] - (mean0[planted] + cfg['shift'])) <= 0.25 * sd0[planted])


# ----------------------------------------------------------------------------------------- the pure parts of learn_alt_model
def _fake_result(L):
    n = 16
    res = dict(n_positions=np.arange(n, dtype=np.int64), n_used=np.full(n, 5000, np.int64), n_outside=np.arange(n, dtype=np.int64) * 2,
               pi=np.full(n, 0.3), mu_mod=np.full(n, 1.0), sd_mod=np.full(n, 0.25), llr=np.full(n, 99.5), iters=np.full(n, 12, np.int32),
               status=np.zeros(n, np.uint8))
    mean0, sd0 = np.full(n, 0.5), np.full(n, 0.2)
    res['status'][1] = L.KMIX_DEGENERATE; res['status'][2] = L.KMIX_TOO_FEW; res['status'][3] = L.KMIX_NO_MODEL
    res['status'][4] = L.KMIX_NOT_CONVERGED; res['status'][5] = L.KMIX_VAR_FLOORED
    res['n_used'][6] = 999; res['n_used'][7] = 1000
    res['pi'][8] = 0.049; res['pi'][9] = 0.05; res['pi'][10] = np.nan
    res['mu_mod'][11] = 0.5 + 0.19; res['mu_mod'][12] = 0.5 - 0.25; res['mu_mod'][13] = np.nan
    return res, mean0, sd0


def test_selection_rule():
    from nanomod_amd import kmermodel
    L, _ = _lib()
    res, mean0, sd0 = _fake_result(L)
    kept = kmermodel.select_alt_codes(res, mean0, sd0, 1000, 0.05, 1.0)
    assert list(np.flatnonzero(~kept)) == [1, 2, 3, 6, 8, 10, 11, 13]          # NOT_CONVERGED and VAR_FLOORED do not exclude a code
    assert kmermodel.select_alt_codes(res, mean0, sd0, 0, 0.0, 0.0).sum() == 16 - 3 - 2   # the status and the NaN estimates still do


def test_alt_model_round_trip_and_table_format():
    from nanomod_amd import kmermodel
    L, _ = _lib()
    res, mean0, sd0 = _fake_result(L)
    kept = kmermodel.select_alt_codes(res, mean0, sd0)
    model = dict(k=2, center=1, mean=mean0, sd=sd0)
    alt = kmermodel.alt_model_from(model, res, kept)
    assert set(alt) == set(kmermodel.KMER_MODEL_FIELDS)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'alt_kmer_model.npz')
        kmermodel.save_kmer_model(path, alt)
        back = kmermodel.load_kmer_model(path)
        for f in kmermodel.KMER_MODEL_FIELDS:
            assert np.array_equal(np.asarray(back[f]), np.asarray(alt[f]), equal_nan=True), f
        assert int(back['k']) == 2 and int(back['center']) == 1 and float(back['clip_sigma']) == 0.0
        assert np.isnan(back['mean'][~kept]).all() and np.isnan(back['sd'][~kept]).all()
        assert np.array_equal(back['mean'][kept], res['mu_mod'][kept]) and np.array_equal(back['sd'][kept], res['sd_mod'][kept])
        assert np.array_equal(back['n_samples'], res['n_used']) and np.array_equal(back['n_clipped'], res['n_outside'])
        table = dict(res, mean0=mean0, sd0=sd0, kept=kept)
        txt = os.path.join(d, 'x_kmer_mix.txt')
        kmermodel.write_kmer_mix_table(txt, model, table)
        lines = open(txt).read().splitlines()
    assert len(kmermodel.KMER_MIX_COLUMNS) == 13 and len(lines) == 16
    assert lines[0] == 'AA 0 5000 0 0.500000 0.200000 0.300000 1.000000 0.250000 99.500 12 0 1'
    assert lines[3] == 'AT 3 5000 6 0.500000 0.200000 0.300000 1.000000 0.250000 99.500 12 4 0'
    assert lines[13].split()[7] == 'nan' and lines[15].split()[0] == 'TT'


def test_listed_rows_match_chrom_strand_and_position():
    from nanomod_amd import kmermodel
    g = dict(chrom=np.array(['a', 'a', 'b', 'b']), strand=np.array(['+', '-', '+', '+']), pos=np.array([5, 5, 5, 6]))
    sites = (np.array(['a', 'b', 'c']), np.array(['-', '+', '+']), np.array([5, 6, 5]))
    assert list(kmermodel._listed_rows(g, sites)) == [False, True, False, True]
    assert not kmermodel._listed_rows(g, (np.zeros(0, str), np.zeros(0, str), np.zeros(0, np.int64))).any()


def test_kmermix_argument_checks_print_error_lines(capsys):
    from nanomod_amd import cli
    with tempfile.TemporaryDirectory() as d:
        rc = cli.main(['kmermix', '--wrkBase1', os.path.join(d, 'no.npz'), '--kmerModel', os.path.join(d, 'no_model.npz'), '--MinCoverage', '2',
                       '--minSamples', '1', '--minPi', '1.5', '--minShift', '-1', '--maxIter', '0', '--tol', '-1', '--sites',
                       os.path.join(d, 'no_sites.txt')])
    out = capsys.readouterr().out.splitlines()
    assert rc == 1 and len(out) == 9 and all(line.startswith('Error: ') for line in out)
    for word in ('--MinCoverage', '--minSamples', '--minPi', '--minShift', '--maxIter', '--tol', 'no.npz', 'no_model.npz', 'no_sites.txt'):
        assert any(word in line for line in out), word
    helps = [a.help for name in ('readllr', 'readdiff', 'readpairs')
             for a in cli.build_parser()._subparsers._group_actions[0].choices[name]._actions if '--altModel' in a.option_strings]
    assert len(helps) == 3 and all("'kmermodel'" in h and "'kmermix'" in h for h in helps)
