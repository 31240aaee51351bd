"""nmod_one_sample (K9) without a GPU: the declaration, the argument checks (before any device work), the numpy restatement of
the definition against scipy, the profile container and position matching, and the command line."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest
from scipy import stats

import one_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine


def _lib():
    import nanomod_amd._lib as L
    return L, L.load()


def test_one_sample_is_declared_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, 'include', 'nanomod_hip.h')).read()
    assert 'nmod_one_sample' in set(re.findall(r'\b(nmod_[a-z0-9_]+)\s*\(', header))
    assert 'nmod_one_sample' in L._SIGNATURES and hasattr(lib, 'nmod_one_sample')
    assert 'NMOD_STATUS_BAD_REFERENCE = 32' in header and L.STATUS_BAD_REFERENCE == 32 == R.BAD_REFERENCE
    assert '#define NMOD_MAX_ONE 16384' in header and '#define NMOD_MAX_ONE_F64 8192' in header
    assert (L.MAX_ONE, L.MAX_ONE_F64) == (16384, 8192) == (R.MAX_ONE, R.MAX_ONE_F64)
    assert (L.STATUS_T_NAN, L.STATUS_EMPTY, L.STATUS_TOO_LARGE, L.STATUS_NONFINITE) == (R.T_NAN, R.EMPTY, R.TOO_LARGE, R.NONFINITE)
    assert C.sizeof(L.NmodOneOut) == 88 and L.NmodOneOut.ks_d.offset == 8 and L.NmodOneOut.status.offset == 80
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # a purely additive entry


def _call(lib, L, npos=4, *, sig='x', off='x', mu='x', sd='x', ref_n=None, run='x', out='x', dtype=None, method=None, nb=2,
          stride=0, wdif=2.0, memspace=None, prm=None, want_comb=True, struct_size=None):
    n = max(npos, 1) if 0 <= npos < 1000 else 4
    x = np.zeros(n * 8, np.float32)
    offs = np.arange(n + 1, dtype=np.int64) * 8
    ref = np.ones(n)
    rid = np.zeros(n, np.int32)
    res = np.zeros(n)
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    o = L.make_one_out(ks_d=res.ctypes.data, ks_p=res.ctypes.data)
    if want_comb:
        o.comb_st = o.comb_p = res.ctypes.data
    if struct_size is not None:
        o.struct_size = struct_size
    if prm is None:
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace,
                            dtype=L.DTYPE_F32 if dtype is None else dtype, method=L.METHOD_STOUFFER if method is None else method,
                            nb=nb, weights_dif=wdif, stride0=stride)
    return lib.nmod_one_sample(C.byref(prm), npos, pick(sig, x), pick(off, offs), pick(mu, ref), pick(sd, ref), pick(ref_n, ref),
                               pick(run, rid), C.byref(o) if out is not None else None)


def test_invalid_arguments_are_refused_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    L, lib = _lib()
    assert _call(lib, L) == -5                                                  # the well-formed call reaches the device check
    assert _call(lib, L, memspace=L.MEM_DEVICE) == -5
    assert _call(lib, L, off=None, stride=8) == -5 and _call(lib, L, ref_n=np.full(4, 9, np.int32)) == -5
    assert _call(lib, L, 0) == 0 and _call(lib, L, 0, sig=None, mu=None, sd=None, off=None) == 0     # npos == 0: NMOD_OK
    assert _call(lib, L, -1) == -1 and _call(lib, L, 2 ** 32 - 1) == -1
    assert _call(lib, L, out=None) == -1 and _call(lib, L, struct_size=80) == -1
    assert _call(lib, L, sig=None) == -1 and _call(lib, L, mu=None) == -1 and _call(lib, L, sd=None) == -1
    assert _call(lib, L, off=None) == -1                                        # neither offsets nor a stride
    assert _call(lib, L, dtype=3) == -1 and _call(lib, L, dtype=-1) == -1
    assert _call(lib, L, nb=-1) == -1 and _call(lib, L, nb=L.MAX_NB + 1) == -1 and _call(lib, L, nb=L.MAX_NB) == -5 and _call(lib, L, nb=0) == -5
    assert _call(lib, L, method=3) == -1 and _call(lib, L, method=-1) == -1
    assert _call(lib, L, off=np.array([0, 8, 4, 12, 16], np.int64)) == -1       # host offsets that decrease
    assert _call(lib, L, off=np.array([-1, 8, 9, 12, 16], np.int64)) == -1
    assert _call(lib, L, run=None) == -1                                        # a combined track without run ids
    assert _call(lib, L, run=None, method=L.METHOD_KS) == -5 and _call(lib, L, run=None, want_comb=False) == -5
    assert _call(lib, L, wdif=0.0) == -1 and _call(lib, L, wdif=0.0, method=L.METHOD_FISHER) == -5
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert _call(lib, L, prm=bad) == -1
    assert lib.nmod_one_sample(None, 4, None, None, None, None, None, None, None) == -1


def test_python_layers_report_the_missing_device_and_bad_shapes():
    import nanomod_amd
    from nanomod_amd import engine
    x, off = np.zeros(8, np.float32), np.array([0, 4, 8], np.int64)
    with pytest.raises(nanomod_amd._lib.NanomodLibraryError, match='nmod_one_sample'):
        engine.one_sample_host(x, off, np.zeros(2), np.ones(2), device=NO_SUCH_DEVICE, method='ks')
    with pytest.raises(ValueError):
        engine.one_sample_host(x, off, np.zeros(2), np.ones(3), device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.one_sample_host(x.astype(np.int32), off, np.zeros(2), np.ones(2), device=NO_SUCH_DEVICE)
    with pytest.raises(ValueError):
        engine.one_sample_host(x, np.array([0, 4, 9], np.int64), np.zeros(2), np.ones(2), device=NO_SUCH_DEVICE)
    assert nanomod_amd.one_sample_host is engine.one_sample_host and nanomod_amd.mtest1 is nanomod_amd.onesample.mtest1


@pytest.mark.parametrize('n', [2, 5, 10, 20, 50, 200, 1000])
def test_reference_against_scipy(n):
    """one_ref on heavily tied rows (3-decimal grid): D against scipy.stats.ks_1samp within 4e-16 absolute (one ulp of 1 is
    2.2e-16: the two sides round the argument of the normal CDF differently), the t pairs against ttest_ind_from_stats(equal_var=
    False) and ttest_1samp within 1e-13 relative.  The rows are shifted by 0 or 0.05 (a quarter of their spread), not by the 0.3 of
    the GPU batches: in the tail d ln p / d ln t is about -t^2, so two correctly rounded t one ulp apart (the definition forms the
    variance as s2 n / (n - 1), scipy with ddof = 1) give p-values t^2 x 2.2e-16 apart, and 1e-13 can only be asked where |t| < 21;
    at n = 1000 a shift of 0.3 is t = 46."""
    rng = np.random.default_rng(1000 + n)
    rows, mu, sd, nr = R.grid_rows(rng, [n] * 50, shift_of=lambda i: 0.0 if i % 2 == 0 else 0.05)
    worst = 0.0
    for i, r in enumerate(R.as_doubles(rows)):
        if np.all(r == r[0]):
            continue
        got = R.position(r, mu[i], sd[i], int(nr[i]))
        model = R.position(r, mu[i], sd[i])
        d = stats.ks_1samp(r, stats.norm(mu[i], sd[i]).cdf).statistic
        worst = max(worst, abs(got['ks_d'] - d))
        assert abs(got['ks_d'] - d) <= 4e-16 and got['ks_d'] == model['ks_d'] and got['ks_p'] == model['ks_p']
        vx, vr = np.var(r) * n / (n - 1.0), sd[i] ** 2 * nr[i] / (nr[i] - 1.0)
        w = stats.ttest_ind_from_stats(np.mean(r), np.sqrt(vx), n, mu[i], np.sqrt(vr), int(nr[i]), equal_var=False)
        o = stats.ttest_1samp(r, mu[i])
        for (t, p), ref in (((got['t_t'], got['t_p']), w), ((model['t_t'], model['t_p']), o)):
            assert abs(t - ref.statistic) <= 1e-13 * abs(ref.statistic) + 1e-300 and abs(p - ref.pvalue) <= 1e-13 * ref.pvalue + 1e-300
        assert np.sign(got['t_t']) == np.sign(np.mean(r) - mu[i]) == np.sign(got['shift'])        # sample minus reference
    print('n = %d: worst |D - ks_1samp| = %.3g' % (n, worst))


def test_reference_statuses():
    x = np.array([0.1, 0.2, 0.35, 0.2])
    assert R.position(x[:0], 0.0, 1.0)['status'] == R.EMPTY
    assert R.position(np.zeros(R.MAX_ONE + 1), 0.0, 1.0)['status'] == R.TOO_LARGE and R.position(np.zeros(R.MAX_ONE), 0.1, 1.0)['status'] == R.T_NAN
    for mu, sd, nr in ((0.0, 0.0, None), (0.0, -1.0, None), (0.0, float('nan'), None), (float('inf'), 1.0, None), (0.0, 1.0, 1)):
        r = R.position(x, mu, sd, nr)
        assert r['status'] == R.BAD_REFERENCE and all(np.isnan(r[k]) for k in R.FIELDS)
    r = R.position(np.array([0.1, float('nan'), 0.3]), 0.0, 1.0)
    assert r['status'] == R.NONFINITE and all(np.isnan(r[k]) for k in R.FIELDS)
    one = R.position(x[:1], 0.0, 1.0, 9)
    assert one['status'] == R.T_NAN and np.isnan(one['t_t']) and np.isnan(one['t_p']) and 0.0 < one['ks_p'] <= 1.0
    same = R.position(np.full(6, 0.25), 0.2, 0.1)
    assert same['status'] == R.T_NAN and same['ks_d'] > 0.0 and R.position(np.full(6, 0.25), 0.2, 0.1, 9)['status'] == 0
    far = R.position(np.full(400, 5.0), 0.0, 0.1)
    assert far['ks_d'] == 1.0 and far['ks_p'] == R.DBL_MIN


def _group(rng, positions, n_of):
    """a per-position container of the given (chrom, strand, pos) list"""
    rows = [np.rint(1000.0 * rng.normal(0.0, 0.2, n_of(i))) / 1000.0 for i in range(len(positions))]
    sig, off = R.csr(rows)
    return dict(chrom=np.array([p[0] for p in positions]), strand=np.array([p[1] for p in positions]),
                pos=np.array([p[2] for p in positions], dtype=np.int64), base=np.array(['ACGT'[p[2] % 4] for p in positions]), off=off, sig=sig)


def test_profile_round_trip_and_matching():
    from nanomod_amd import onesample
    rng = np.random.default_rng(5)
    pos = [('chr2', '+', p) for p in range(100, 110)] + [('chr1', '-', p) for p in range(7, 12)] + [('chr1', '+', p) for p in (3, 4, 9)]
    n = rng.integers(3, 40, len(pos)).astype(np.int32)
    prof = onesample.make_profile([p[0] for p in pos], [p[1] for p in pos], [p[2] for p in pos], ['ACGT'[p[2] % 4] for p in pos],
                                  rng.normal(size=len(pos)), rng.uniform(0.1, 0.4, len(pos)), n)
    # the reference's order: sorted (chrom, strand), '+' before '-', ascending position
    keys = [(str(prof['chrom_names'][c]), str(s), int(p)) for c, s, p in zip(prof['chrom_id'], prof['strand'], prof['pos'])]
    assert keys == sorted(pos, key=lambda k: (k[0], k[1] == '-', k[2])) and prof['kind'] == 'control'
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'p.npz')
        onesample.save_profile(path, prof)
        back = onesample.load_profile(path)
        assert set(back) == set(onesample.PROFILE_FIELDS) == set(prof)
        assert all(np.array_equal(back[k], prof[k]) for k in prof) and back['mean'].dtype == np.float64 and back['n'].dtype == np.int32
        model = onesample.make_profile([p[0] for p in pos], [p[1] for p in pos], [p[2] for p in pos], ['A'] * len(pos),
                                       np.zeros(len(pos)), np.ones(len(pos)))
        onesample.save_profile(path, model)
        back_m = onesample.load_profile(path)
        assert back_m['kind'] == 'model' and 'n' not in back_m and 'n' not in np.load(path).files
        broken = dict(model, kind='control')
        with pytest.raises(ValueError):
            onesample.save_profile(path, broken)

    # matching: the sample group misses chr1 '+' 9, has one position the profile lacks, and two thin rows
    gpos = [p for p in keys if p != ('chr1', '+', 9)] + [('chr3', '+', 1)]
    thin_g = {('chr2', '+', 104), ('chr1', '-', 8)}
    g = _group(rng, gpos, lambda i: 3 if gpos[i] in thin_g else 12)
    lines = []
    meta, sig, off, mu, sd, ref_n, rid = onesample.match_positions(g, prof, 5, lambda *a: lines.append(' '.join(map(str, a))))
    thin_p = {k for k, c in zip(keys, prof['n']) if c < 5}
    want = [k for k in keys if k in set(gpos) and k not in thin_g and k not in thin_p]
    got = [(str(c), str(s), int(p)) for c, s, p in zip(meta['chrom'], meta['strand'], meta['pos'])]
    assert got == want and len(want) < len(keys) - 1
    idx = [keys.index(k) for k in want]
    assert np.array_equal(mu, prof['mean'][idx]) and np.array_equal(sd, prof['sd'][idx]) and np.array_equal(ref_n, prof['n'][idx])
    assert np.array_equal(meta['n0'], np.full(len(want), 12)) and np.array_equal(meta['n1'], ref_n) and len(sig) == off[-1] == 12 * len(want)
    from nanomod_amd import detect
    assert np.array_equal(rid, detect.run_ids(meta['chrom'], meta['strand'], meta['pos']))
    assert len(lines) == 1 and '%d position(s) tested' % len(want) in lines[0]
    assert '%d of the sample group dropped (2 below MinCoverage' % (len(gpos) - len(want)) in lines[0]
    assert '%d of the profile dropped (%d below MinCoverage' % (len(keys) - len(want), len(thin_p)) in lines[0]
    # a model has no coverage of its own: only the sample's counts
    meta_m, _, _, _, _, ref_n_m, _ = onesample.match_positions(g, model, 5, lambda *a: None)
    assert ref_n_m is None and not meta_m['n1'].any() and len(meta_m['pos']) == len([k for k in keys if k in set(gpos) and k not in thin_g])


def test_cli_parser():
    from nanomod_amd import cli
    p = cli.build_parser()
    a = p.parse_args(['profile', '--wrkBase1', 'g.npz', '--MinCoverage', '7', '--outFolder', 'd', '--FileID', 'id'])
    assert (a.cmd, a.wrkBase1, a.MinCoverage, a.outFolder, a.FileID) == ('profile', 'g.npz', 7, 'd', 'id')
    a = p.parse_args(['detect1', '--wrkBase1', 'g.npz', '--refProfile', 'p.npz', '--MinCoverage', '9', '--neighborPvalues', '3',
                      '--WeightsDif', '1.5', '--testMethod', 'fisher', '--rankUse', 'st', '--topN', '4', '--fdr', 'by', '--fdrAlpha', '0.1',
                      '--device', '1', '--outFolder', 'o', '--FileID', 'f', '--SaveTest', '0', '--Pos', 'chr1:100'])
    assert (a.cmd, a.refProfile, a.MinCoverage, a.neighborPvalues, a.WeightsDif, a.testMethod, a.rankUse, a.topN, a.fdr, a.fdrAlpha,
            a.device, a.outFolder, a.FileID, a.SaveTest, a.Pos) == ('detect1', 'p.npz', 9, 3, 1.5, 'fisher', 'st', 4, 'by', 0.1, 1, 'o', 'f', 0, 'chr1:100')
    for argv in (['detect1', '--wrkBase1', 'g.npz'], ['profile'], ['detect', '--wrkBase1', 'g.npz'], ['detect1', '--wrkBase1', 'g', '--refProfile', 'p', '--wrkBase2', 'h']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    assert cli.main(['detect1', '--wrkBase1', '/nonexistent/g.npz', '--refProfile', '/nonexistent/p.npz']) == 1
    assert cli.main(['profile', '--wrkBase1', '/nonexistent/g.npz', '--MinCoverage', '2']) == 1
