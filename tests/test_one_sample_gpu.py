"""-m gpu: nmod_one_sample (K9) against tests/one_ref.py, its own invariants, nmod_combine_track, and the two-sample path.
Gates (from the issue of this feature, reasoned there): ks_d 1e-13 absolute (erfc is within 16 ulp, 1.8e-15 on values <= 1);
ks_p / t_p the project's 1e-9 relative gate (helpers.assert_close_p); t_t, shift, mean, std 1e-11 relative + 1e-12 absolute (the
header's bound for the Welch t of both moment forms); status bits equal."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
from scipy import stats

import helpers as H
import one_ref as R

pytestmark = pytest.mark.gpu

# the size classes of one_sample.hip (kOneSmall, kOneWave, kOneWave2) and the caps: every edge, a few rows of each
EDGES = (1, 2, 3, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
PER_SIZE = 3


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _sizes(dtype):
    cap = R.MAX_ONE_F64 if dtype == 'f64' else R.MAX_ONE
    return [n for n in EDGES + (cap, cap + 1) for _ in range(PER_SIZE)], cap


_edge_cache = {}


def _edge_batch(dtype):
    """the class-edge batch of a dtype and its one_ref results with and without ref_n: computed once, never changed"""
    if dtype not in _edge_cache:
        sizes, cap = _sizes(dtype)
        rows16, mu, sd, nr = R.grid_rows(np.random.default_rng(42), sizes)
        rows = R.as_dtype(rows16, dtype)
        dbl = R.as_doubles(rows)
        _edge_cache[dtype] = (rows, mu, sd, nr, cap, {True: R.batch(dbl, mu, sd, nr, cap), False: R.batch(dbl, mu, sd, None, cap)})
    return _edge_cache[dtype]


def _compare(res, ref, what):
    assert np.array_equal(res['status'], ref['status']), (what, np.flatnonzero(res['status'] != ref['status'])[:8])
    nan = np.isnan(ref['ks_d'])
    assert np.array_equal(np.isnan(res['ks_d']), nan)
    err = np.abs(res['ks_d'][~nan] - ref['ks_d'][~nan])
    print('%s: max |ks_d - ref| = %.3g' % (what, err.max() if err.size else 0.0))
    assert (err <= 1e-13).all(), (what, err.max())
    H.assert_close_p(res['ks_p'], ref['ks_p'], 1e-9, what + ' ks_p')
    H.assert_close_p(res['t_p'], ref['t_p'], 1e-9, what + ' t_p')
    for k in ('t_t', 'shift', 'mean', 'std'):
        H.assert_close_stat(res[k], ref[k], 1e-11, 1e-12, what + ' ' + k)


@pytest.mark.parametrize('with_n', [True, False])
@pytest.mark.parametrize('dtype', ['f32', 'i16', 'f64'])
def test_class_edges_against_reference(nm, dtype, with_n):
    rows, mu, sd, nr, cap, ref = _edge_batch(dtype)
    sig, off = R.csr(rows)
    res = nm.engine.one_sample_host(sig, off, mu, sd, nr if with_n else None, method='ks')
    _compare(res, ref[with_n], '%s %s' % (dtype, 'control' if with_n else 'model'))
    big = np.diff(off) > cap
    assert big.sum() == PER_SIZE and (res['status'][big] == R.TOO_LARGE).all() and all(np.isnan(res[k][big]).all() for k in R.FIELDS)
    assert (res["status"][~big] & 0xFD == 0).all() and (res['status'][np.diff(off) == 1] == R.T_NAN).all()


def test_edge_rows(nm):
    """degenerate rows between ordinary ones; the neighbours are what they are alone"""
    L = nm._lib
    rng = np.random.default_rng(7)
    plain = lambda n=40: np.rint(1000.0 * rng.normal(0.1, 0.2, n)) / 1000.0
    far = 0.1 + 50 * 0.2 + 0.001 * rng.integers(0, 5, 800)
    rows = [plain(), np.full(30, 0.25), plain(), far, plain(), np.zeros(0), plain(), np.r_[plain(300), np.nan], plain(),
            np.r_[np.inf, plain(20)], plain(), plain(), plain(), plain(), plain(), plain(), plain()]
    npos = len(rows)
    mu, sd, nr = np.full(npos, 0.1), np.full(npos, 0.2), np.full(npos, 50, np.int32)
    bad = {11: ('sd', 0.0), 12: ('sd', -0.2), 13: ('sd', np.nan), 14: ('mu', np.inf), 15: ('nr', 1)}
    for i, (k, v) in bad.items():
        {'sd': sd, 'mu': mu, 'nr': nr}[k][i] = v
    sig, off = R.csr(rows)
    for dtype in (np.float64, np.float32):
        s = sig.astype(dtype)
        dbl = [np.asarray(r, dtype).astype(np.float64) for r in rows]
        for with_n in (True, False):
            ref_n = nr if with_n else None
            res = nm.engine.one_sample_host(s, off, mu, sd, ref_n, method='ks')
            _compare(res, R.batch(dbl, mu, sd, ref_n), 'edge rows')
            st = res['status']
            assert st[1] == (0 if with_n else L.STATUS_T_NAN) and 0.0 < res['ks_p'][1] < 1.0 and res['std'][1] == 0.0      # all samples equal
            assert res['ks_d'][3] == 1.0 and res['ks_p'][3] == R.DBL_MIN
            assert st[5] == L.STATUS_EMPTY and st[7] == L.STATUS_NONFINITE == st[9]
            expect_bad = [i for i, (k, _) in bad.items() if k != 'nr' or with_n]
            assert all(st[i] == L.STATUS_BAD_REFERENCE for i in expect_bad) and (with_n or st[15] == 0)
            for i in [5, 7, 9] + expect_bad:
                assert all(np.isnan(res[k][i]) for k in R.FIELDS)
            for i in (0, 2, 4, 6, 8, 10, 16):                       # ordinary neighbours: the bits of the position alone
                one = nm.engine.one_sample_host(s[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]]), mu[i:i + 1], sd[i:i + 1],
                                                None if ref_n is None else ref_n[i:i + 1], method='ks')
                assert st[i] == 0 and all(one[k][0].tobytes() == res[k][i].tobytes() for k in R.FIELDS)
    # the clamp is nmod_detect_batch's: two groups 800 v 800 that do not overlap have D = 1 and a tail below DBL_MIN too
    a, b = np.zeros(800, np.float32), np.ones(800, np.float32)
    two = nm.engine.detect_host(a, None, b, None, np.zeros(1, np.int32), method='ks', tests=L.TEST_KS, stride0=800, stride1=800)
    assert two['ks_d'][0] == 1.0 and two['ks_p'][0] == R.DBL_MIN == res['ks_p'][3]


@pytest.mark.parametrize('method', ['stouffer', 'fisher'])
@pytest.mark.parametrize('nb', [0, 2])
def test_combine_is_the_window_combine_of_the_ks_track(nm, nb, method):
    rng = np.random.default_rng(11)
    npos = 61
    rows = [np.rint(1000.0 * rng.normal(0.0, 0.2, 50)) / 1000.0 for _ in range(npos)]
    rows[20] = np.r_[rows[20][:-1], np.nan]                       # a NaN position inside the second run
    rows[40] = rows[40] + 1.0                                     # and a strong one in the third
    mu, sd = rng.normal(0.0, 0.05, npos), np.full(npos, 0.2)
    rid = np.repeat(np.arange(3, dtype=np.int32), [13, 20, 28])
    sig, off = R.csr(rows)
    res = nm.engine.one_sample_host(sig.astype(np.float32), off, mu, sd, None, rid, nb=nb, method=method)
    st, pv = nm.engine.combine_host(res['ks_d'], res['ks_p'], rid, nb=nb, method=method)
    assert res['comb_st'].tobytes() == st.tobytes() and res['comb_p'].tobytes() == pv.tobytes()
    assert np.isnan(res['ks_p'][20]) and np.isnan(res['comb_p'][20]) and np.isfinite(res['comb_p'][rid != 1]).all()
    if nb:
        assert np.isnan(res['comb_p'][18:23]).all() and not np.isnan(res['comb_p'][[17, 23]]).any()


def test_combine_is_not_written_for_method_ks(nm):
    L, lib = nm._lib, nm._lib.load()
    x, off = np.linspace(-0.3, 0.3, 40).astype(np.float32), np.array([0, 20, 40], np.int64)
    mu, sd, rid = np.zeros(2), np.full(2, 0.2), np.zeros(2, np.int32)
    ks_d, comb = np.zeros(2), np.full(4, -7.0)
    o = L.make_one_out(ks_d=ks_d.ctypes.data, comb_st=comb[:2].ctypes.data, comb_p=comb[2:].ctypes.data)
    prm = L.make_params(memspace=L.MEM_HOST, dtype=L.DTYPE_F32, method=L.METHOD_KS, nb=2)
    assert lib.nmod_one_sample(C.byref(prm), 2, x.ctypes.data, off.ctypes.data, mu.ctypes.data, sd.ctypes.data, None, rid.ctypes.data, C.byref(o)) == 0
    assert (comb == -7.0).all() and (ks_d > 0.0).all()
    assert 'comb_p' not in nm.engine.one_sample_host(x, off, mu, sd, method='ks')


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_every_position_alone_gives_the_same_bits(nm, dtype):
    rows, mu, sd, nr, cap, _ = _edge_batch(dtype)
    sig, off = R.csr(rows)
    res = nm.engine.one_sample_host(sig, off, mu, sd, nr, method='ks')
    for i in range(0, len(rows)):
        one = nm.engine.one_sample_host(rows[i], np.array([0, len(rows[i])]), mu[i:i + 1], sd[i:i + 1], nr[i:i + 1], method='ks')
        assert all(one[k][0].tobytes() == res[k][i].tobytes() for k in R.FIELDS + ('status',)), (i, len(rows[i]))


def test_stride_host_device_and_dtype_forms_agree_bit_for_bit(nm):
    import torch
    rows16, mu, sd, nr = R.grid_rows(np.random.default_rng(3), [200] * 64)
    rid = np.repeat(np.arange(4, dtype=np.int32), 16)
    keys = R.FIELDS + ('comb_st', 'comb_p', 'status')
    by_dtype = {}
    for dtype in ('i16', 'f64', 'f32'):
        sig, off = R.csr(R.as_dtype(rows16, dtype))
        a = nm.engine.one_sample_host(sig, off, mu, sd, nr, rid)
        b = nm.engine.one_sample_host(sig, None, mu, sd, nr, rid, stride=200)
        assert all(a[k].tobytes() == b[k].tobytes() for k in keys), dtype          # stride form == CSR form
        det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer')
        dev = lambda v: torch.from_numpy(v).cuda()
        c = det.one_sample(dev(sig), dev(mu), dev(sd), dev(nr), dev(rid), off=dev(off))
        d = det.one_sample(dev(sig), dev(mu), dev(sd), dev(nr), dev(rid), stride=200)
        torch.cuda.synchronize()
        for r in (c, d):                                                           # NMOD_MEM_HOST == NMOD_MEM_DEVICE
            assert all(a[k].tobytes() == r[k].cpu().numpy().tobytes() for k in keys), dtype
        by_dtype[dtype] = a
    # int16 rows and the same values as float64 k / 1000.0: the same order statistics, evaluated by the same function
    assert all(by_dtype['i16'][k].tobytes() == by_dtype['f64'][k].tobytes() for k in ('ks_d', 'ks_p', 'comb_st', 'comb_p'))
    # beyond the wave-resident classes too (the workgroup form of both)
    rows16, mu, sd, nr = R.grid_rows(np.random.default_rng(4), [3000, 5000, 8192])
    big = {dt: nm.engine.one_sample_host(*R.csr(R.as_dtype(rows16, dt)), mu, sd, nr, method='ks') for dt in ('i16', 'f64')}
    assert all(big['i16'][k].tobytes() == big['f64'][k].tobytes() for k in ('ks_d', 'ks_p'))


def test_against_the_two_sample_path(nm):
    """512 positions x 200 v 200 event rows, group 2 planted +0.3 at positions 0, 1, 15 mod 16.  The profile of group 2, then group 1
    against it with ref_n: the Welch t of the two-sample call on the full data, the profile's moments its mean1 / std1, the planted
    positions found.  The seed is the first from 20241017 on for which every |t| of the two-sample reference (scipy on the CPU
    restatement of the rows) is above 0.01: a mean near the level 3 is only defined to an ulp, 4.4e-16, which is 2.2e-14 in t at a
    standard error of 0.02, so "1e-11 relative" means something only where |t| >> 2e-3 — the project's own t gate adds that absolute
    floor (helpers.t_abs_gate), this test keeps the issue's purely relative one and rows on which it is meaningful.
    Uniformity of the unplanted KS p-values: the one-sample KS takes the reference as exact, and a control of the SAME depth
    doubles the variance of the level difference — tests/one_ref.py alone (CPU, no device code) rejects uniformity at the 1e-4
    level over all 416 unplanted positions (p = 1e-13), so, as the issue of this feature prescribes, the row count is lowered and
    the level kept: the first 64 unplanted positions (reference: p = 0.12).  Against the generator's own level and spread as a
    MODEL, where nothing is estimated, all 512 positions of group 1 (never planted) are uniform at that level (reference: p = 0.60)."""
    import torch
    npos, n, seed = 512, 200, 20241026
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=nm._lib.TEST_KS | nm._lib.TEST_WELCH, want_mstd=True)
    sig0 = torch.empty(npos * n, dtype=torch.int16, device='cuda:0'); sig1 = torch.empty_like(sig0)
    det.synth_fill_events(sig0, seed, 0, npos, 0, n_per_pos=n, plant_period=16, plant_shift_milli=300, spread_milli=200)
    det.synth_fill_events(sig1, seed, 0, npos, 1, n_per_pos=n, plant_period=16, plant_shift_milli=300, spread_milli=200)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    two = {k: v.cpu().numpy() for k, v in det.run(sig0, sig1, rid, stride0=n, stride1=n, npos=npos).items()}
    h0, h1 = sig0.cpu().numpy(), sig1.cpu().numpy()
    assert np.array_equal(h0.reshape(npos, n), H.synth_events_ref(seed, 0, npos, 0, n, 16, 300, 200, 'i16'))
    group2 = dict(chrom=np.full(npos, 'chr1'), strand=np.full(npos, '+'), pos=np.arange(npos, dtype=np.int64), base=np.full(npos, 'A'),
                  off=np.arange(npos + 1, dtype=np.int64) * n, sig=h1)
    prof = nm.build_profile(group2, 5, 0)
    assert prof['kind'] == 'control' and (prof['n'] == n).all() and np.array_equal(prof['pos'], group2['pos'])
    H.assert_close_stat(prof['mean'], two['mean1'], 1e-12, 0.0, 'profile mean')
    H.assert_close_stat(prof['sd'], two['std1'], 1e-12, 0.0, 'profile sd')
    one = nm.engine.one_sample_host(h0, None, prof['mean'], prof['sd'], prof['n'], rid.cpu().numpy(), stride=n)
    assert not one['status'].any() and np.array_equal(np.sign(one['t_t']), np.sign(two['t_t']))
    H.assert_close_stat(one['t_t'], two['t_t'], 1e-11, 0.0, 't_t against the two-sample Welch t')
    H.assert_close_p(one['t_p'], two['t_p'], 1e-9, 't_p against the two-sample Welch t')
    mm = np.arange(npos) % 16
    planted = (mm == 0) | (mm == 1) | (mm == 15)
    assert np.median(one['ks_p'][planted]) < 1e-6 and (one['shift'][planted] < -1.0).all()
    un = np.flatnonzero(~planted)[:64]
    assert stats.kstest(one['ks_p'][un], 'uniform').pvalue >= 1e-4
    pos = np.arange(npos, dtype=np.int64)[:, None]
    lev = (H._mix64(np.uint64(seed) ^ np.uint64(0xA5A5A5A5DEADBEEF), pos, 0, np.zeros((1, 1), np.uint64)) >> np.uint64(40)) % np.uint64(6001)
    model = nm.engine.one_sample_host(h0, None, (lev.astype(np.int64).reshape(-1) - 3000) / 1000.0, np.full(npos, 0.2), method='ks', stride=n)
    assert stats.kstest(model['ks_p'], 'uniform').pvalue >= 1e-4


def test_device_entry_composes_with_fdr(nm):
    """DeviceDetector.one_sample -> .fdr on its tracks in plain stream order, nothing synchronised or read in between; the host
    entries on the same rows give the same bits, and the pool gives the scratch back"""
    import torch
    npos, n, seed = 4096, 200, 5
    det = nm.DeviceDetector(0, nb=2, weights_dif=2.0, method='fisher')
    sig = torch.empty(npos * n, dtype=torch.int16, device='cuda:0')
    det.synth_fill_events(sig, seed, 0, npos, 1, n_per_pos=n, plant_period=64, plant_shift_milli=400, spread_milli=200)
    h = sig.cpu().numpy().reshape(npos, n)
    mm = np.arange(npos) % 64
    planted = (mm == 0) | (mm == 1) | (mm == 63)
    mu = (np.median(h, axis=1) - np.where(planted, 400, 0)) / 1000.0
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    rid = np.zeros(npos, np.int32)
    d_mu, d_sd, d_rid = dev(mu), dev(np.full(npos, 0.2)), dev(rid)

    def whole():
        res = det.one_sample(sig, d_mu, d_sd, None, d_rid, stride=n)
        qs, summ = det.fdr(res, tracks=('ks_p', 't_p', 'comb_p'), method='bh', alpha=0.01)
        torch.cuda.synchronize()
        return res, qs, summ
    res, qs, summ = whole()
    host = nm.engine.one_sample_host(h.reshape(-1), None, mu, np.full(npos, 0.2), None, rid, stride=n, method='fisher')
    assert all(host[k].tobytes() == res[k].cpu().numpy().tobytes() for k in host)
    hq, _ = nm.engine.fdr_adjust_host([host['ks_p'], host['t_p'], host['comb_p']], method='bh', alpha=0.01)
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(hq, qs))
    assert (qs[0].cpu().numpy()[planted] <= 0.01).all()
    assert [s['tested'] for s in nm.engine.fdr_summary_dicts(summ)] == [npos] * 3

    def settle():
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        assert nm._lib.load().nmod_trim_scratch(0) == 0
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]
    free0 = settle()
    del res, qs, summ
    whole()
    assert free0 - settle() <= (2 << 20)


def test_cli_profile_then_detect1(nm, capsys):
    from nanomod_amd import cli, container, onesample
    from test_abi_and_host import _fixture_containers
    with tempfile.TemporaryDirectory() as tmp:
        p0, p1 = _fixture_containers('g50', tmp)
        out = os.path.join(tmp, 'out')
        assert cli.main(['profile', '--wrkBase1', p1, '--MinCoverage', '5', '--outFolder', out, '--FileID', 'ctl']) == 0
        ppath = os.path.join(out, 'ctl_profile.npz')
        prof = onesample.load_profile(ppath)
        g0, g1 = container.load_group(p0), container.load_group(p1)
        assert prof['kind'] == 'control' and len(prof['pos']) == int((np.diff(g1['off']) >= 5).sum()) > 0
        assert cli.main(['detect1', '--wrkBase1', p0, '--refProfile', ppath, '--outFolder', out, '--FileID', 'run', '--fdr', 'bh',
                         '--topN', '3', '--outLevel', '3']) == 0
        printed = capsys.readouterr().out
        meta, sig, off, mu, sd, ref_n, rid = onesample.match_positions(g0, prof, 5, lambda *a: None)
        npos = len(rid)
        assert npos > 10 and np.array_equal(np.lexsort((meta['pos'], meta['strand'] == '-', meta['chrom'])), np.arange(npos))   # reference order
        res = nm.engine.one_sample_host(sig, off, mu, sd, ref_n, rid, nb=2, weights_dif=2.0, method='stouffer')
        want = ''.join('%s %s %d %s %d %d %.3f %.3f %.3E %.3f %.3E %.3f %.3E\n' % (
            meta['chrom'][i], meta['strand'][i], meta['pos'][i] + 1, meta['base'][i], meta['n0'][i], ref_n[i], res['shift'][i], res['t_t'][i],
            res['t_p'][i], res['ks_d'][i], res['ks_p'][i], res['comb_st'][i], res['comb_p'][i]) for i in range(npos))
        assert open(os.path.join(out, 'run_one_sample.txt')).read() == want
        lines = open(os.path.join(out, 'run_one_sample_fdr.txt')).read().splitlines()
        assert len(lines) == npos
        for col, key in enumerate(('t_p', 'ks_p', 'comb_p')):
            ok = (res[key] >= 0.0) & (res[key] <= 1.0)
            q = np.full(npos, np.nan)
            q[ok] = stats.false_discovery_control(res[key][ok], method='bh')
            assert [ln.split()[4 + col] for ln in lines] == ['%.3E' % v for v in q], key
        assert [ln.split()[:4] for ln in lines] == [ln.split()[:4] for ln in want.splitlines()]
        best = np.lexsort((res['ks_p'], res['comb_p']))[0]
        assert printed.splitlines()[-3].split()[:4] == ['1', str(meta['chrom'][best]), str(meta['strand'][best]), str(meta['pos'][best] + 1)]
