"""nmod_kmer_model (K10) on the device against tests/kmer_ref.py.

Gates: counts and pos_status exact; int16 mean / sd within 1e-14 relative of the exact rational value (the formula makes fewer than
ten roundings of 1.1e-16 on exact integers); float mean / sd within the project's moment gate, 1e-11 relative + 1e-12 absolute;
int16 bits equal under any permutation of the positions."""
import os
import tempfile

import numpy as np
import pytest

import kmer_ref as R
from helpers import assert_close_stat

pytestmark = pytest.mark.gpu

DTYPES = {'i16': np.int16, 'f32': np.float32, 'f64': np.float64}
COUNTS = ('n_positions', 'n_samples', 'n_clipped')
# the issue's row lengths, and the int16 kernel's own edges: a lane's piece of 8 samples, a wave's step of 512
EDGE_LENGTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4097]


def _engine():
    from nanomod_amd import engine
    return engine


def _check(got, exp, dtype, name=''):
    for k in COUNTS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], exp[k]), (name, k)
    assert np.array_equal(got['pos_status'], exp['pos_status']), (name, 'pos_status')
    for k in ('mean', 'sd'):
        g, e = got[k], exp[k]
        assert np.array_equal(np.isnan(g), np.isnan(e)), (name, k, 'NaN pattern')
        m = ~np.isnan(e)
        if np.dtype(dtype) == np.int16:
            err = np.abs(g[m] - e[m])
            assert (err <= 1e-14 * np.abs(e[m])).all(), (name, k, float(err.max()))
        else:
            assert_close_stat(g, e, rel=1e-11, abs_=1e-12, name='%s %s' % (name, k))


def _bits_equal(a, b, keys=COUNTS + ('mean', 'sd', 'pos_status'), rows=None):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if rows is not None and k != 'pos_status':
            x, y = x[rows], y[rows]
        assert x.tobytes() == y.tobytes(), k


@pytest.fixture(scope='module')
def edge_rows():
    """three rows of every edge length, in a shuffled order, among 2 200 short rows (1 .. 11 samples): 2 266 positions are more
    than two workgroups of the int16 kernel (1 024 positions each) and no multiple of its tile of 64"""
    rng = np.random.default_rng(2024)
    lengths = np.array(EDGE_LENGTHS * 3 + rng.integers(1, 12, 2200).tolist())
    lengths = lengths[rng.permutation(len(lengths))]
    levels = rng.normal(0.0, 1.0, len(lengths))
    k = R.grid_rows(rng, lengths.tolist(), lambda i: levels[i], dtype=np.int16)
    return {name: [r if dt == np.int16 else (r.astype(np.float64) / 1000.0).astype(dt) for r in k] for name, dt in DTYPES.items()}


@pytest.mark.parametrize('ncodes', [1, 4, 64, 4096, 65536])
@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_class_edges(edge_rows, dt, ncodes):
    """random codes in [-1, ncodes): the LDS table (up to 4 096 codes) and the global one; milli-grid rows with 1 % outliers"""
    rows, dtype = edge_rows[dt], DTYPES[dt]
    rng = np.random.default_rng(ncodes)
    codes = rng.integers(-1, ncodes, len(rows)).astype(np.int32)
    if ncodes >= 64:
        codes[codes == 7] = 8                                               # some codes are absent
        codes[(codes > ncodes // 2) & (codes % 3 == 0)] = 5
    sig, off = R.csr(rows, dtype)
    got = _engine().kmer_model_host(sig, off, codes, ncodes)
    exp = R.kmer_model(rows, codes, ncodes, dtype)
    _check(got, exp, dtype, '%s ncodes=%d' % (dt, ncodes))
    assert exp['n_positions'].sum() == (codes >= 0).sum() and (ncodes < 64 or exp['n_samples'][7] == 0)


def test_one_deep_row_needs_64_bit_sums():
    """70 000 samples of +32 767 under code 0: S1 = 2.29e9 is beyond 2^31, S2 = 7.5e13 beyond 2^32; and a row of -32 768"""
    rng = np.random.default_rng(7)
    rows = R.grid_rows(rng, [5, 9, 70000, 3, 12, 200, 1001], lambda i: 0.3, dtype=np.int16)
    rows[2] = np.full(70000, 32767, np.int16)
    rows[6] = np.full(1001, -32768, np.int16)                               # two squares of these are 2^31
    codes = np.array([1, 0, 0, 2, 1, 0, 3], np.int32)
    sig, off = R.csr(rows, np.int16)
    got = _engine().kmer_model_host(sig, off, codes, 4)
    _check(got, R.kmer_model(rows, codes, 4, np.int16), np.int16, 'deep')
    alone = _engine().kmer_model_host(rows[2], np.array([0, 70000], np.int64), np.zeros(1, np.int32), 1)
    assert alone['n_samples'][0] == 70000 and alone['mean'][0] == 32.767 and alone['sd'][0] == 0.0


@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_clip_bounds_are_inclusive_and_a_nan_bound_keeps_nothing(dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(31)
    lengths = [3, 20, 64, 9, 130, 5, 77, 8, 600, 11, 40, 2]
    rows = R.grid_rows(rng, lengths, lambda i: 0.1 * (i % 3), dtype=dtype)
    codes = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 4, 4], np.int32)
    ncodes = 6
    # code 0: bounds exactly on two sample values of its rows (as the doubles the definition takes them as); code 1: unbounded
    # below; code 2: every sample clipped; code 3: a NaN bound; code 4: lo == hi on one sample; code 5: no positions
    xs0 = sorted(R.as_double(x, dtype) for x in np.concatenate([rows[0], rows[4], rows[8]]).tolist())
    one4 = R.as_double(rows[10][0], dtype)
    lo = np.array([xs0[len(xs0) // 4], -np.inf, 40.0, np.nan, one4, 0.0])
    hi = np.array([xs0[3 * len(xs0) // 4], 0.1, 50.0, 1.0, one4, 1.0])
    sig, off = R.csr(rows, dtype)
    got = _engine().kmer_model_host(sig, off, codes, ncodes, lo, hi)
    exp = R.kmer_model(rows, codes, ncodes, dtype, lo, hi)
    _check(got, exp, dtype, 'clip ' + dt)
    pooled0 = np.array(xs0)
    assert got['n_samples'][0] == int(((pooled0 >= lo[0]) & (pooled0 <= hi[0])).sum()) and (pooled0 == lo[0]).any() and (pooled0 == hi[0]).any()
    for c in (2, 3):                                                        # nothing kept: N = 0, NaN, no position counted
        assert got['n_samples'][c] == 0 and got['n_positions'][c] == 0 and np.isnan(got['mean'][c]) and np.isnan(got['sd'][c])
        assert got['n_clipped'][c] == sum(len(rows[i]) for i in range(len(rows)) if codes[i] == c)
    assert got['n_samples'][4] >= 1 and (dt != 'i16' or (got['mean'][4] == one4 and got['sd'][4] == 0.0))
    assert not got['pos_status'].any()                                      # clipping drops samples, never positions
    swapped = _engine().kmer_model_host(sig, off, codes, ncodes, hi, lo)    # lo > hi keeps nothing (code 4: lo == hi still does)
    assert swapped['n_samples'][0] == 0 and swapped['n_samples'][4] == got['n_samples'][4]


def test_sigma_clipping_through_build_kmer_model():
    """clip_sigma = 3 with two rounds equals the reference's three sequential passes"""
    from nanomod_amd import kmermodel
    rng = np.random.default_rng(77)
    n = 400
    chrom = np.array(['chr1'] * n); strand = np.array(['+'] * (n // 2) + ['-'] * (n // 2))
    pos = np.concatenate([np.arange(n // 2), np.arange(n // 2)]).astype(np.int64)
    base = rng.choice(list('ACGT'), n)
    k, center, ncodes = 2, 1, 16
    codes = R.kmer_codes(chrom, strand, pos, base, k, center)
    level = rng.normal(0.0, 1.0, ncodes)
    lengths = rng.integers(3, 40, n)
    rows = R.grid_rows(rng, lengths.tolist(), lambda i: level[max(codes[i], 0)], outliers=0.03, dtype=np.int16)
    sig, off = R.csr(rows, np.int16)
    group = dict(chrom=chrom, strand=strand, pos=pos, base=base, off=off, sig=sig.astype(np.float64) / 1000.0)
    lines = []
    model = kmermodel.build_kmer_model(group, k, center, min_coverage=5, clip_sigma=3.0, clip_rounds=2, log=lambda *a: lines.append(' '.join(map(str, a))))
    used = np.where(lengths >= 5, codes, -1).astype(np.int32)
    exp = R.kmer_model(rows, used, ncodes, np.int16)
    plain = exp
    for _ in range(2):
        have = np.isfinite(exp['mean']) & np.isfinite(exp['sd'])
        lo = np.where(have, exp['mean'] - 3.0 * exp['sd'], -np.inf); hi = np.where(have, exp['mean'] + 3.0 * exp['sd'], np.inf)
        exp = R.kmer_model(rows, used, ncodes, np.int16, lo, hi)
    got = dict(model, pos_status=exp['pos_status'])
    _check(got, exp, np.int16, 'sigma clipping')
    assert exp['n_clipped'].sum() > 0 and (exp['sd'][exp['n_samples'] > 0] <= plain['sd'][exp['n_samples'] > 0]).all()
    assert int(model['k']) == k and int(model['center']) == center and float(model['clip_sigma']) == 3.0 and len(model['mean']) == ncodes
    assert len(lines) == 1 and '%d below MinCoverage' % int(((lengths < 5) & (codes >= 0)).sum()) in lines[0]
    assert '%d without a full k-mer' % int((codes < 0).sum()) in lines[0]


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_nonfinite_rows_are_dropped_whole(dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(5)
    lengths = [6, 70, 9, 300, 4, 4, 17, 5, 8, 64]
    rows = R.grid_rows(rng, lengths, lambda i: 0.0, dtype=dtype)
    codes = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 3], np.int32)
    sig, off = R.csr(rows, dtype)
    clean = _engine().kmer_model_host(sig, off, codes, 4)
    bad = [r.copy() for r in rows]
    bad[1][69] = np.nan; bad[3][0] = np.inf; bad[4][2] = -np.inf
    sig_b, _ = R.csr(bad, dtype)
    got = _engine().kmer_model_host(sig_b, off, codes, 4)
    exp = R.kmer_model(bad, codes, 4, dtype)
    _check(got, exp, dtype, 'nonfinite ' + dt)
    assert got['pos_status'].tolist() == [0, 16, 0, 16, 16, 0, 0, 0, 0, 0]
    _bits_equal(got, clean, keys=COUNTS + ('mean', 'sd'), rows=[2, 3])      # the codes without a bad row are unchanged
    # a bound that would clip the bad sample does not save the position
    got_c = _engine().kmer_model_host(sig_b, off, codes, 4, np.full(4, -100.0), np.full(4, 100.0))
    assert np.array_equal(got_c['pos_status'], got['pos_status']) and np.array_equal(got_c['n_samples'], got['n_samples'])


@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_empty_rows_and_missing_codes(dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(9)
    lengths = [5, 0, 7, 0, 12, 3, 0, 66, 9]
    rows = R.grid_rows(rng, lengths, lambda i: 0.2, dtype=dtype)
    codes = np.array([0, 0, -1, -1, 1, 1, 2, 2, -1], np.int32)
    sig, off = R.csr(rows, dtype)
    got = _engine().kmer_model_host(sig, off, codes, 3)
    _check(got, R.kmer_model(rows, codes, 3, dtype), dtype, 'status ' + dt)
    assert got['pos_status'].tolist() == [0, 4, 64, 64 | 4, 0, 0, 4, 0, 64]
    assert got['n_positions'].tolist() == [1, 2, 1] and got['n_samples'].tolist() == [5, 15, 66]
    none = _engine().kmer_model_host(sig, off, np.full(len(rows), -1, np.int32), 3)      # nothing takes part
    assert not none['n_samples'].any() and np.isnan(none['mean']).all() and (none['pos_status'] & 64).all()


@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_out_of_range_codes_in_device_memory(dt):
    """NMOD_STATUS_NO_CODE, and nothing is written outside the tables"""
    import torch
    from nanomod_amd import DeviceDetector
    dtype = DTYPES[dt]
    rng = np.random.default_rng(13)
    lengths = rng.integers(1, 30, 200).tolist()
    rows = R.grid_rows(rng, lengths, lambda i: 0.1, dtype=dtype)
    ncodes = 5
    codes = rng.integers(0, ncodes, 200).astype(np.int32)
    wild = codes.copy()
    wild[[3, 50, 51, 120, 199]] = [ncodes, ncodes + 5, -7, 2 ** 31 - 1, -2 ** 31]
    codes[[3, 50, 51, 120, 199]] = -1
    sig, off = R.csr(rows, dtype)
    exp = _engine().kmer_model_host(sig, off, codes, ncodes)
    det = DeviceDetector(0)
    dev = 'cuda:0'
    guard = {k: torch.full((ncodes + 2,), -99, dtype=torch.int64, device=dev) for k in COUNTS}
    guard.update({k: torch.full((ncodes + 2,), -99.0, dtype=torch.float64, device=dev) for k in ('mean', 'sd')})
    guard['pos_status'] = torch.full((len(rows) + 2,), 255, dtype=torch.uint8, device=dev)
    out = {k: t[1:-1] for k, t in guard.items()}
    res = det.kmer_model(torch.from_numpy(sig).to(dev), torch.from_numpy(wild).to(dev), ncodes, off=torch.from_numpy(off).to(dev), out=out)
    torch.cuda.synchronize()
    got = {k: t.cpu().numpy() for k, t in res.items()}
    _bits_equal(got, exp)
    assert (got['pos_status'][[3, 50, 51, 120, 199]] == 64).all()
    for k, t in guard.items():
        edge = t.cpu().numpy()[[0, -1]]
        assert (edge == (255 if k == 'pos_status' else -99)).all(), k


@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_layout_and_memspace_do_not_change_the_bits(dt):
    """CSR versus stride, host versus device memory, and a second run"""
    import torch
    from nanomod_amd import DeviceDetector
    dtype = DTYPES[dt]
    rng = np.random.default_rng(17)
    npos, n, ncodes = 1500, 37, 20
    rows = R.grid_rows(rng, [n] * npos, lambda i: 0.01 * (i % 50), dtype=dtype)
    codes = rng.integers(-1, ncodes, npos).astype(np.int32)
    sig, off = R.csr(rows, dtype)
    lo, hi = np.full(ncodes, -0.3), np.full(ncodes, 0.6)
    for bounds in ((None, None), (lo, hi)):
        host_csr = _engine().kmer_model_host(sig, off, codes, ncodes, *bounds)
        host_stride = _engine().kmer_model_host(sig, None, codes, ncodes, *bounds, stride=n)
        _bits_equal(host_csr, host_stride)
        _bits_equal(host_csr, _engine().kmer_model_host(sig, off, codes, ncodes, *bounds))
        det = DeviceDetector(0)
        t = lambda a: None if a is None else torch.from_numpy(a).to('cuda:0')
        # (a sample vector that starts 2 bytes into an allocation: rows begin at any even address)
        shifted = torch.empty(len(sig) + 1, dtype=t(sig).dtype, device='cuda:0')
        shifted[1:] = t(sig)
        d_csr = det.kmer_model(shifted[1:], t(codes), ncodes, t(bounds[0]), t(bounds[1]), off=t(off))
        d_stride = det.kmer_model(t(sig), t(codes), ncodes, t(bounds[0]), t(bounds[1]), stride=n)
        torch.cuda.synchronize()
        _bits_equal(host_csr, {k: v.cpu().numpy() for k, v in d_csr.items()})
        _bits_equal(host_csr, {k: v.cpu().numpy() for k, v in d_stride.items()})


@pytest.mark.parametrize('dt', ['i16', 'f32', 'f64'])
def test_other_codes_in_the_batch_do_not_change_a_codes_bits(dt):
    dtype = DTYPES[dt]
    rng = np.random.default_rng(19)
    lengths = rng.integers(1, 90, 700).tolist()
    rows = R.grid_rows(rng, lengths, lambda i: 0.05 * (i % 7), dtype=dtype)
    codes = rng.integers(0, 4, 700).astype(np.int32)
    sig, off = R.csr(rows, dtype)
    alone = _engine().kmer_model_host(sig, off, codes, 8)
    others = R.grid_rows(rng, rng.integers(1, 200, 900).tolist(), lambda i: 1.0, dtype=dtype)
    slot = np.sort(rng.integers(0, 701, 900))                               # others[j] goes in front of rows[slot[j]]
    mixed, mixed_codes, j = [], [], 0
    for i in range(701):
        while j < 900 and slot[j] == i:
            mixed.append(others[j]); mixed_codes.append(4 + j % 4); j += 1
        if i < 700:
            mixed.append(rows[i]); mixed_codes.append(int(codes[i]))
    sig_m, off_m = R.csr(mixed, dtype)
    both = _engine().kmer_model_host(sig_m, off_m, np.array(mixed_codes, np.int32), 8)
    _bits_equal(alone, both, keys=COUNTS + ('mean', 'sd'), rows=[0, 1, 2, 3])
    assert both['n_positions'][4:].sum() == 900 and not alone['n_positions'][4:].any()


def test_int16_bits_do_not_depend_on_the_order_of_the_positions():
    rng = np.random.default_rng(23)
    lengths = rng.integers(1, 300, 1200).tolist()
    rows = R.grid_rows(rng, lengths, lambda i: 0.02 * (i % 31), dtype=np.int16)
    for ncodes in (50, 5000):                                               # the LDS table and the global one
        codes = rng.integers(-1, ncodes, 1200).astype(np.int32)
        lo, hi = np.full(ncodes, -0.25), np.full(ncodes, 0.75)
        sig, off = R.csr(rows, np.int16)
        first = _engine().kmer_model_host(sig, off, codes, ncodes, lo, hi)
        perm = rng.permutation(1200)
        sig_p, off_p = R.csr([rows[i] for i in perm], np.int16)
        second = _engine().kmer_model_host(sig_p, off_p, codes[perm], ncodes, lo, hi)
        _bits_equal(first, second, keys=COUNTS + ('mean', 'sd'))
        assert np.array_equal(first['pos_status'][perm], second['pos_status']) and first['n_clipped'].sum() > 0


def test_end_to_end_model_to_one_sample_detection():
    """a control of 40 reads gives the 3-mer table; a sample of the same sequence with +1.0 planted at three positions is tested
    against the table's prediction, through the Python layers and through the command line"""
    from nanomod_amd import cli, container, detect, engine, kmermodel, onesample
    rng = np.random.default_rng(2025)
    nb_, k, center = 3000, 3, 1
    chrom = np.array(['chr1'] * (2 * nb_)); strand = np.array(['+'] * nb_ + ['-'] * nb_)
    pos = np.concatenate([np.arange(nb_), np.arange(nb_)]).astype(np.int64)
    base = rng.choice(list('ACGT'), 2 * nb_)
    codes = R.kmer_codes(chrom, strand, pos, base, k, center)
    level = rng.normal(0.0, 1.0, 4 ** k)
    truth = level[np.maximum(codes, 0)]

    def group(reads, plant=()):
        x = np.rint(1000.0 * (truth[:, None] + rng.normal(0.0, 0.2, (2 * nb_, reads))))
        for i in plant:
            x[i] += 1000.0
        return dict(chrom=chrom, strand=strand, pos=pos, base=base, off=np.arange(2 * nb_ + 1, dtype=np.int64) * reads, sig=x.ravel() / 1000.0)

    control = group(40)
    model = kmermodel.build_kmer_model(control, k, center, min_coverage=5, log=lambda *a: None)
    assert (model['n_positions'] > 0).all() and model['n_positions'].sum() == (codes >= 0).sum() == 2 * nb_ - 4
    assert (np.abs(model['mean'] - level) <= 5.0 * model['sd'] / np.sqrt(model['n_samples'])).all()
    assert (np.abs(model['sd'] - 0.2) < 0.02).all()

    planted = [700, 1500, nb_ + 2200]                                       # away from the run edges
    sample = group(50, planted)
    prof = kmermodel.model_profile(model, sample)
    assert prof['kind'] == 'model' and len(prof['pos']) == 2 * nb_ - 4
    with tempfile.TemporaryDirectory() as tmp:
        mo = {'ds2': ['s'], 's': {'nmod_container': sample}, 'nmod_profile': prof, 'MinCoverage': 5, 'neighborPvalues': 2, 'WeightsDif': 2.0,
              'testMethod': 'stouffer', 'rankUse': 'pv', 'SaveTest': 1, 'outFolder': os.path.join(tmp, 'py'), 'FileID': 'e2e', 'outLevel': 3,
              'nmod_quiet': 1}
        onesample.mtest1(mo)
        res, meta = mo['one_sample_arrays'], mo['one_sample_meta']
        rows = np.flatnonzero(codes >= 0)
        assert np.array_equal(meta['pos'], pos[rows]) and np.array_equal(meta['strand'], strand[rows])
        want = set(int(np.flatnonzero(rows == i)[0]) for i in planted)
        for key in ('ks_p', 't_p'):
            assert set(np.argsort(res[key], kind='stable')[:3].tolist()) == want, key
        # the table's entries, fed directly
        sig_r, off_r = container.gather_rows(sample['sig'], sample['off'], rows)
        direct = engine.one_sample_host(onesample._encode(sig_r), off_r, model['mean'][codes[rows]], model['sd'][codes[rows]], None,
                                        detect.run_ids(chrom[rows], strand[rows], pos[rows]), nb=2, weights_dif=2.0, method='stouffer')
        assert set(direct) == set(res)
        for key in direct:
            assert np.asarray(direct[key]).tobytes() == np.asarray(res[key]).tobytes(), key
        # the command line: kmermodel -> kmerprofile -> detect1
        c_path, s_path, out = os.path.join(tmp, 'control.npz'), os.path.join(tmp, 'sample.npz'), os.path.join(tmp, 'cli')
        container.save_group(c_path, **{f: control[f] for f in ('chrom', 'strand', 'pos', 'base', 'off', 'sig')})
        container.save_group(s_path, **{f: sample[f] for f in ('chrom', 'strand', 'pos', 'base', 'off', 'sig')})
        assert cli.main(['kmermodel', '--wrkBase1', c_path, '--kmer', '3', '--kmerCenter', '1', '--outFolder', out, '--FileID', 'ctl', '--outLevel', '3']) == 0
        back = kmermodel.load_kmer_model(os.path.join(out, 'ctl_kmer_model.npz'))
        assert all(np.asarray(back[f]).tobytes() == np.asarray(model[f]).tobytes() for f in kmermodel.KMER_MODEL_FIELDS)
        table = open(os.path.join(out, 'ctl_kmer_model.txt')).read().splitlines()
        assert len(table) == 64 and table[0] == 'AAA %d %d %.6f %.6f' % (model['n_positions'][0], model['n_samples'][0], model['mean'][0], model['sd'][0])
        assert cli.main(['kmerprofile', '--kmerModel', os.path.join(out, 'ctl_kmer_model.npz'), '--wrkBase1', s_path, '--outFolder', out,
                         '--FileID', 'smp', '--outLevel', '3']) == 0
        assert cli.main(['detect1', '--wrkBase1', s_path, '--refProfile', os.path.join(out, 'smp_profile.npz'), '--outFolder', out,
                         '--FileID', 'e2e', '--outLevel', '3', '--topN', '3']) == 0
        assert open(os.path.join(out, 'e2e_one_sample.txt')).read() == open(os.path.join(tmp, 'py', 'e2e_one_sample.txt')).read()
